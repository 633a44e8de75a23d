// The run-time-shape W = 256 instances of the 48-point forward kernel (mlp_fused48_kernel.h: DN_FWD48_W256_RT).
#include "mlp_fused48_kernel.h"
namespace dn { DN_FWD48_W256_RT(DN_FWD48_INSTANTIATE) }
