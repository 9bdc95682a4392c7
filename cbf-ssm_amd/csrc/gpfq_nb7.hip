#include "cbfssm_gp_fullq.hpp"
CBF_GPFQ_INSTANTIATE(7)
