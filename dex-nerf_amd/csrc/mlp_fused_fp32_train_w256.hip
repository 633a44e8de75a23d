// The fp32 training-forward instances of the W = 256 nets of the 32-point forward kernel (mlp_fused_kernel.h: DN_FWD32_FP32_TRAIN_W256);
// launched from mlp_fused.hip dispatch_forward.
#include "mlp_fused_kernel.h"
namespace dn { DN_FWD32_FP32_TRAIN_W256(DN_FWD32_INSTANTIATE) }
