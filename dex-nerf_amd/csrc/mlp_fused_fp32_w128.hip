// The fp32 instances (training forward and inference) of the W = 128 nets of the 32-point forward kernel (mlp_fused_kernel.h:
// DN_FWD32_FP32_W128); launched from mlp_fused.hip dispatch_forward.
#include "mlp_fused_kernel.h"
namespace dn { DN_FWD32_FP32_W128(DN_FWD32_INSTANTIATE) }
