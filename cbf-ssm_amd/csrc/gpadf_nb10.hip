#include "cbfssm_gp_adf.hpp"
CBF_GPADF_INSTANTIATE(10)
