// The self-compositing instances of the paper network of the 48-point forward kernel (mlp_fused48_kernel.h: DN_FWD48_PAPER_COMP).
#include "mlp_fused48_kernel.h"
namespace dn { DN_FWD48_PAPER_COMP(DN_FWD48_INSTANTIATE) }
