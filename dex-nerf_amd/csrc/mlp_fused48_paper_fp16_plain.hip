// The explicit-schedule fp16 instance of the paper network (D8 / W256 / skip 4, view directions) of the 48-point forward kernel,
// plain form: every tile encoded at its top (mlp_fused48_kernel.h: DN_FWD48_PAPER_FP16_PLAIN); launched from mlp_fused48.hip
// launch_forward48.  One instance per unit: its tile pass is compiled once per wave role.
#include "mlp_fused48_kernel.h"
namespace dn { DN_FWD48_PAPER_FP16_PLAIN(DN_FWD48_INSTANTIATE) }
