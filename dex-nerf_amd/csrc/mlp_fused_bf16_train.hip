// The bf16 training-forward instances of the 32-point forward kernel (mlp_fused_kernel.h: DN_FWD32_BF16_TRAIN);
// launched from mlp_fused.hip dispatch_forward.
#include "mlp_fused_kernel.h"
namespace dn { DN_FWD32_BF16_TRAIN(DN_FWD32_INSTANTIATE) }
