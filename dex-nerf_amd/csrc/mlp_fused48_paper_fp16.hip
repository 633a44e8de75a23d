// The explicit-schedule fp16 instance of the paper network (D8 / W256 / skip 4, view directions) of the 48-point forward kernel on
// rays + depths, the next tile's encoding inside the view-direction stage (mlp_fused48_kernel.h: DN_FWD48_PAPER_FP16_ENC); launched
// from mlp_fused48.hip launch_forward48.  One instance per unit: its tile pass is compiled once per wave role.
#include "mlp_fused48_kernel.h"
namespace dn { DN_FWD48_PAPER_FP16_ENC(DN_FWD48_INSTANTIATE) }
