#include "cbfssm_gp_rollout.hpp"
CBF_GPROLL_INSTANTIATE(7)
