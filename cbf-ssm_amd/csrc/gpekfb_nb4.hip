#include "cbfssm_gp_ekf_bwd.hpp"
CBF_GPEKFBWD_INSTANTIATE(4)
