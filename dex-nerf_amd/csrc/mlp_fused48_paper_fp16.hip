// The explicit-schedule fp16 instances of the paper network (D8 / W256 / skip 4, view directions) of the 48-point forward kernel
// (mlp_fused48_kernel.h: DN_FWD48_PAPER_FP16); launched from mlp_fused48.hip launch_forward48.
#include "mlp_fused48_kernel.h"
namespace dn { DN_FWD48_PAPER_FP16(DN_FWD48_INSTANTIATE) }
