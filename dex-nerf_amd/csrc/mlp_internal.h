// Host-side helpers shared between mlp_fused.hip (packing, forward dispatch, inference entry points; the forward kernel itself is
// mlp_fused_kernel.h, compiled in mlp_fused_*.hip), mlp_train.hip (training forward / backward-data entry points) and mlp_wgrad.hip
// (weight gradients).
#pragma once
#include "mlp_device.h"

namespace dn {

struct PackPtrs {
  const float* w[kMaxStages];
  const float* b[kMaxStages];
};

int setup_params(const dn_mlp_desc* desc, int precision, const void* packed, FwdParams* p);
struct CompParams;
int dispatch_forward(const dn_mlp_desc& d, int precision, FwdParams& p, hipStream_t stream, const CompParams* comp = nullptr, int* composited = nullptr);
int launch_pack(const NetLayout& L, const PackPtrs& ptrs, void* packed, int precision, hipStream_t stream, bool density = false);

}  // namespace dn
