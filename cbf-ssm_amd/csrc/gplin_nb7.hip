#include "cbfssm_gp_lin.hpp"
CBF_GPLIN_INSTANTIATE(7)
