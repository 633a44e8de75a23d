// Host-only check of the 48-point forward's instance selection (mlp_geo48.h g48_pick): over the cross product of descriptors,
// precisions, inference / training, input modes, samples per ray, launch sizes and switch settings, every key returned is a row of
// DN_FWD48_INSTANCES / DN_FWD48_DENSITY (mlp_fused48_kernel.h) and every row is returned at least once.  Launches nothing.
#include "mlp_fused48_kernel.h"
#include <cstdio>
#include <vector>

using namespace dn;

namespace dn { void set_error(const char*, ...) {} }   // (referenced by inline helpers of the headers; never called here)

struct Row { G48Key key; bool density; long hits; };

static dn_mlp_desc net(int W, int D, int skip, int lxyz, int viewdirs) {
  dn_mlp_desc d{};
  d.num_layers = D; d.hidden_size = W; d.skip_connect_every = skip; d.num_encoding_fn_xyz = lxyz; d.num_encoding_fn_dir = 4;
  d.include_input_xyz = 1; d.include_input_dir = 1; d.use_viewdirs = viewdirs; d.log_sampling_xyz = 1; d.log_sampling_dir = 1;
  return d;
}

int main() {
  std::vector<Row> rows;
#define DN_ROW(W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP) rows.push_back(Row{G48Key{W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP}, false, 0});
  DN_FWD48_INSTANCES(DN_ROW)
#undef DN_ROW
#define DN_ROW(W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP) rows.push_back(Row{G48Key{W, F, DC, MASKC, VIEWC, SAVE, OVLP, COMP}, true, 0});
  DN_FWD48_DENSITY(DN_ROW)
#undef DN_ROW
  std::vector<dn_mlp_desc> nets;
  for (int lxyz : {10, 6})
    for (int viewdirs : {1, 0}) {
      nets.push_back(net(256, 8, 4, lxyz, viewdirs));   // paper trunk
      nets.push_back(net(128, 4, 4, lxyz, viewdirs));   // as-shipped trunk
      nets.push_back(net(256, 8, 3, lxyz, viewdirs));   // W 256, another skip pattern
      nets.push_back(net(128, 3, 4, lxyz, viewdirs));   // W 128, another depth
    }
  const int cus = 256;
  const long long sizes[] = {50 * 24, 1024 * 64, 4096 * 64};   // render-sized; two point groups (256 of 256-point tiles); three
  char dummy[16];
  float rgb = 0.0f;
  long picks = 0, refusals = 0, unknown = 0;
  for (const dn_mlp_desc& d : nets)
    for (int precision : {DN_PREC_BF16, DN_PREC_F16})
      for (int training = 0; training < 2; ++training)
        for (int save8 = 0; save8 < 2; ++save8)
          for (int mode = 0; mode < 3; ++mode)
            for (int S : {24, 25})
              for (long long n : sizes)
                for (int with_comp = 0; with_comp < 2; ++with_comp)
                  for (int bits = 0; bits < 8; ++bits)
                    for (int groups : {0, 2, 3}) {
                      Switches sw{};
                      sw.runtime_shape = bits & 1; sw.no_overlap = bits & 2; sw.fused_composite = bits & 4; sw.train_groups = groups;
                      FwdParams p{};
                      p.act = training ? dummy : nullptr; p.save8 = save8; p.mode = mode; p.S = S; p.n_points = n / 24 * S;
                      CompParams comp{};
                      comp.rgb = &rgb; comp.n_rays = n / 24;
                      const G48Pick pick = g48_pick(d, precision, p, with_comp ? &comp : nullptr, cus, sw);
                      ++picks;
                      if (pick.refusal) { ++refusals; continue; }
                      bool found = false;
                      for (Row& r : rows)
                        if (r.density == pick.density && r.key == pick.key) { ++r.hits; found = true; }
                      if (!found) {
                        ++unknown;
                        std::printf("not a row: W=%d F=%d DC=%d MASKC=%#x VIEWC=%d SAVE=%d OVLP=%d COMP=%d density=%d\n", pick.key.W, pick.key.F,
                                    pick.key.DC, pick.key.MASKC, pick.key.VIEWC, pick.key.SAVE, pick.key.OVLP, pick.key.COMP, pick.density);
                      }
                    }
  long unreached = 0;
  for (const Row& r : rows)
    if (r.hits == 0) {
      ++unreached;
      std::printf("never picked: W=%d F=%d DC=%d MASKC=%#x VIEWC=%d SAVE=%d OVLP=%d COMP=%d density=%d\n", r.key.W, r.key.F, r.key.DC, r.key.MASKC,
                  r.key.VIEWC, r.key.SAVE, r.key.OVLP, r.key.COMP, r.density);
    }
  std::printf("g48_pick: %ld calls, %ld refusals, %zu rows, %ld unknown keys, %ld unreached rows\n", picks, refusals, rows.size(), unknown, unreached);
  return (unknown || unreached || rows.size() != 26) ? 1 : 0;
}
