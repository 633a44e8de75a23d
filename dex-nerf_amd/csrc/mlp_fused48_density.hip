// The fixed-shape no-view-direction instances of the 48-point forward kernel (mlp_fused48_kernel.h: DN_FWD48_DENSITY): the density
// sub-network of the D8 / W256 / skip-4 and the 4 x 128 nets (dn_mlp_pack_density); launched from mlp_fused48.hip launch_forward48.
// Same template, compiled here under a name of its own.
#define mlp_forward48_kernel mlp_forward_density48_kernel
#include "mlp_fused48_kernel.h"
namespace dn { DN_FWD48_DENSITY(DN_FWD48_INSTANTIATE) }
