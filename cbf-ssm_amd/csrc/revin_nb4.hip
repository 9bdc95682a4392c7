#include "cbfssm_adjoint_inst.hpp"
CBF_REVIN_INSTANTIATE(4)
