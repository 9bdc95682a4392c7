#include "cbfssm_gp_adf_bwd.hpp"
CBF_GPADFB_INSTANTIATE(16)
