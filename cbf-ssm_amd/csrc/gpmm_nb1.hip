#include "cbfssm_gp_mm.hpp"
CBF_GPMM_INSTANTIATE(1)
