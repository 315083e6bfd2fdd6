// The depth gate's pure logic (edge_alignment_amd/csrc/ea_depth_gate.h) on a depth image of 2^s times the DT extent, for the
// host: a stand-alone program that runs gate_point -- what the kernel calls -- over points, a matrix and a depth image read
// from a file and writes class bytes and weights to another; tests/test_depth_gate_scaled_host.py holds them to
// tests/depth_gate_scaled_ref.py byte for byte and bit for bit.  Host compiler only (-ffp-contract=off), no device.
//
// usage: depth_gate_scaled_host IN OUT
// IN:  int32 n, H, W (the DT extent), kind, radius, has_dist, f32, dw_power, shift, pad; double M[12], K[4] (fx fy cx cy),
//      dist[5], z_scaling, abs_tol, rel_tol, w_occluded, w_free, w_unknown, dw_z_ref; n x 3 doubles (the stored points);
//      (H << shift) x (W << shift) samples of the kind.
// OUT: n class bytes, then n doubles (the weights, rounded through float when f32).
// exit: 0 done; 1 usage; 2 IN cannot be read or is refused; 3 OUT cannot be written
#include <stdio.h>

#include <vector>

#include "ea_depth_gate.h"

namespace {
struct Header {
  int32_t n, H, W, kind, radius, has_dist, f32, dw_power, shift, pad;
  double M[12], K[4], dist[5], z_scaling, abs_tol, rel_tol, w_occluded, w_free, w_unknown, dw_z_ref;
};

template <typename RAW, int R>
void run_radius(const Header &h, const ea::DepthGateRule &rule, const double *xyz, const RAW *img, uint8_t *cls, double *w) {
  for (int i = 0; i < h.n; ++i) {
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const int c = ea::gate_point<RAW, R>(h.M, x, y, z, h.K[0], h.K[1], h.K[2], h.K[3], h.has_dist ? h.dist : nullptr, img, h.H, h.W,
                                         h.z_scaling, h.abs_tol, h.rel_tol, h.shift);
    cls[i] = (uint8_t)c;
    const double wi = ea::gate_weight(ea::gate_factor(rule, c), ea::gate_depth_factor(z, h.dw_z_ref, h.dw_power));
    w[i] = h.f32 ? (double)(float)wi : wi;
  }
}

template <typename RAW>
bool run(const Header &h, const double *xyz, const RAW *img, uint8_t *cls, double *w) {
  ea_depth_gate_params prm;
  prm.radius = h.radius; prm.abs_tol = h.abs_tol; prm.rel_tol = h.rel_tol;
  prm.w_occluded = h.w_occluded; prm.w_free = h.w_free; prm.w_unknown = h.w_unknown; prm.apply = 1;
  if (ea::depth_gate_params_error(&prm)) return false;
  const ea::DepthGateRule rule = ea::depth_gate_rule(&prm);
  switch (h.radius) {
    case 0: run_radius<RAW, 0>(h, rule, xyz, img, cls, w); break;
    case 1: run_radius<RAW, 1>(h, rule, xyz, img, cls, w); break;
    case 2: run_radius<RAW, 2>(h, rule, xyz, img, cls, w); break;
    default: run_radius<RAW, 3>(h, rule, xyz, img, cls, w); break;
  }
  return true;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 1;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  Header h;
  std::vector<double> xyz;
  std::vector<uint16_t> u16;
  std::vector<float> f32;
  bool ok = fread(&h, sizeof(h), 1, f) == 1 && h.n >= 0 && h.shift >= 0 && h.shift <= ea::kDepthGateMaxShift &&
            !ea::now_depth_args_error(h.kind, h.H, h.W, h.z_scaling) &&
            ea::depth_gate_shift(h.H, h.W, h.H << h.shift, h.W << h.shift) == h.shift;
  if (ok) {
    const size_t px = ((size_t)h.H << h.shift) * ((size_t)h.W << h.shift);
    xyz.resize((size_t)h.n * 3);
    (h.kind == EA_DEPTH_U16 ? u16.resize(px) : f32.resize(px));
    ok = fread(xyz.data(), sizeof(double), xyz.size(), f) == xyz.size() &&
         (h.kind == EA_DEPTH_U16 ? fread(u16.data(), 2, px, f) == px : fread(f32.data(), 4, px, f) == px);
  }
  fclose(f);
  if (!ok) return 2;
  std::vector<uint8_t> cls((size_t)h.n);
  std::vector<double> w((size_t)h.n);
  if (!(h.kind == EA_DEPTH_U16 ? run(h, xyz.data(), u16.data(), cls.data(), w.data()) : run(h, xyz.data(), f32.data(), cls.data(), w.data())))
    return 2;
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 3;
  ok = fwrite(cls.data(), 1, cls.size(), o) == cls.size() && fwrite(w.data(), sizeof(double), w.size(), o) == w.size();
  return fclose(o) == 0 && ok ? 0 : 3;
}
