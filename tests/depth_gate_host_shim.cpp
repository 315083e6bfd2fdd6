// The depth gate's pure logic (edge_alignment_amd/csrc/ea_depth_gate.h) for the host: the argument checks, and the gate run
// over points, a matrix and a depth image read from a file, behind a C interface that tests/test_depth_gate_host.py loads with
// ctypes and holds to tests/depth_gate_ref.py byte for byte and bit for bit.  Host compiler only, no device.
//
// The file: int32 n, H, W, kind, radius, has_dist, f32, dw_power; double M[12], K[4] (fx fy cx cy), dist[5], z_scaling, abs_tol,
// rel_tol, w_occluded, w_free, w_unknown, dw_z_ref; n x 3 doubles (the stored points); H x W samples of the kind.
#include <stdio.h>

#include <vector>

#include "ea_depth_gate.h"

namespace {
struct Header {
  int32_t n, H, W, kind, radius, has_dist, f32, dw_power;
  double M[12], K[4], dist[5], z_scaling, abs_tol, rel_tol, w_occluded, w_free, w_unknown, dw_z_ref;
};

template <typename RAW>
int run(const Header &h, const double *xyz, const RAW *img, uint8_t *cls, double *w) {
  ea_depth_gate_params prm;
  prm.radius = h.radius; prm.abs_tol = h.abs_tol; prm.rel_tol = h.rel_tol;
  prm.w_occluded = h.w_occluded; prm.w_free = h.w_free; prm.w_unknown = h.w_unknown; prm.apply = 1;
  if (ea::depth_gate_params_error(&prm)) return -1;
  const ea::DepthGateRule rule = ea::depth_gate_rule(&prm);
  for (int i = 0; i < h.n; ++i) {
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    double bz, u, v, d;
    int c, iu, iv;
    ea::gate_project(h.M, x, y, z, h.K[0], h.K[1], h.K[2], h.K[3], h.has_dist ? h.dist : nullptr, &bz, &u, &v);
    if (ea::gate_behind(bz)) c = EA_GATE_BEHIND;
    else if (!ea::gate_inside(u, v, h.H, h.W, &iu, &iv)) c = EA_GATE_OUTSIDE;
    else if (!ea::gate_scan_radius<RAW>(h.radius, img, h.H, h.W, iu, iv, h.z_scaling, bz, &d)) c = EA_GATE_UNKNOWN;
    else c = ea::gate_classify(d, bz, h.abs_tol, h.rel_tol);
    cls[i] = (uint8_t)c;
    const double wi = ea::gate_weight(ea::gate_factor(rule, c), ea::gate_depth_factor(z, h.dw_z_ref, h.dw_power));
    w[i] = h.f32 ? (double)(float)wi : wi;
  }
  return 0;
}
}  // namespace

// 0: done; -1: the parameters are refused; -2: the file cannot be read; -3: capacity too small
extern "C" int depth_gate_file_c(const char *path, uint8_t *cls, double *w, int capacity) {
  FILE *f = fopen(path, "rb");
  if (!f) return -2;
  Header h;
  int rc = -2;
  if (fread(&h, sizeof(h), 1, f) == 1 && h.n >= 0 && !ea::now_depth_args_error(h.kind, h.H, h.W, h.z_scaling)) {
    if (h.n > capacity) rc = -3;
    else {
      std::vector<double> xyz((size_t)h.n * 3);
      const size_t px = (size_t)h.H * (size_t)h.W;
      std::vector<uint16_t> u16(h.kind == EA_DEPTH_U16 ? px : 0);
      std::vector<float> f32(h.kind == EA_DEPTH_F32 ? px : 0);
      const bool ok = fread(xyz.data(), sizeof(double), xyz.size(), f) == xyz.size() &&
                      (h.kind == EA_DEPTH_U16 ? fread(u16.data(), 2, px, f) == px : fread(f32.data(), 4, px, f) == px);
      if (ok) rc = h.kind == EA_DEPTH_U16 ? run(h, xyz.data(), u16.data(), cls, w) : run(h, xyz.data(), f32.data(), cls, w);
    }
  }
  fclose(f);
  return rc;
}

extern "C" int depth_gate_params_ok_c(int radius, double abs_tol, double rel_tol, double w_occluded, double w_free, double w_unknown) {
  ea_depth_gate_params prm = {radius, abs_tol, rel_tol, w_occluded, w_free, w_unknown, 1};
  return ea::depth_gate_params_error(&prm) ? 0 : 1;
}

extern "C" int depth_gate_factors_fit_float_c(double w_occluded, double w_free, double w_unknown) {
  ea_depth_gate_params prm = {0, 0.0, 0.0, w_occluded, w_free, w_unknown, 1};
  return ea::depth_gate_factors_fit(&prm, 3.4028234663852886e38) ? 1 : 0;
}

extern "C" int now_depth_args_ok_c(int kind, int height, int width, double z_scaling) {
  return ea::now_depth_args_error(kind, height, width, z_scaling) ? 0 : 1;
}

extern "C" int depth_gate_header_bytes_c(void) { return (int)sizeof(Header); }
extern "C" int depth_gate_seg_bytes_c(void) { return (int)sizeof(ea::DepthGateSeg); }
