#include "cbfssm_gp_bwd.hpp"
CBF_GPBWD_INSTANTIATE(1)
