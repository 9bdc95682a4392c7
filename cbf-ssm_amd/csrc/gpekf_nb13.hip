#include "cbfssm_gp_ekf.hpp"
CBF_GPEKF_INSTANTIATE(13)
