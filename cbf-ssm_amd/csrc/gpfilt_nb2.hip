#include "cbfssm_gp_filter.hpp"
CBF_GPFILT_INSTANTIATE(2)
