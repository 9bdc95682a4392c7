#include "cbfssm_gp_mm_bwd.hpp"
CBF_GPMMB_INSTANTIATE(13)
