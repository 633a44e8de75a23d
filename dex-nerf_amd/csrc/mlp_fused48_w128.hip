// The W = 128 instances of the 48-point forward kernel (mlp_fused48_kernel.h: DN_FWD48_W128); launched from mlp_fused48.hip launch_forward48.
#include "mlp_fused48_kernel.h"
namespace dn { DN_FWD48_W128(DN_FWD48_INSTANTIATE) }
