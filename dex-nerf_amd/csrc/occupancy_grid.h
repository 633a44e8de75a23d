// What occupancy.hip shares with occupancy_live.hip: the cell rule of the occupancy entry points and the one dilation of raw bit words
// (include/dexnerf_hip_occupancy.h "Build") - dn_occupancy_build and dn_occupancy_ema_update store the same bits for the same raw words.
#pragma once
#include "dn_common.h"

namespace dn {
namespace occ {

struct Cells {
  int cx, cy, cz;
  int64_t n;   // cx * cy * cz
};

// false: cells the entry points refuse
bool cells_of(int cx, int cy, int cz, Cells& g);
int64_t words_of(const Cells& g);

// out[w] = (accumulate ? out[w] : 0) | the OR of raw over the Chebyshev neighbourhood d >= 1 of each of the word's cells; one launch,
// raw != out
void launch_dilate(const unsigned* raw, const Cells& g, int d, int accumulate, unsigned* out, hipStream_t s);

}  // namespace occ
}  // namespace dn
