// The bf16 inference and fp16 render instances of the 32-point forward kernel (mlp_fused_kernel.h: DN_FWD32_BF16);
// launched from mlp_fused.hip dispatch_forward.
#include "mlp_fused_kernel.h"
namespace dn { DN_FWD32_BF16(DN_FWD32_INSTANTIATE) }
