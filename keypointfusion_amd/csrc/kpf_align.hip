// The depth stream registered to the colour camera (sensor.DepthAligner): raw depth frames of the depth sensor in, the colour camera's depth
// image out, uint16 mm on the colour grid.
//   align_clear_kernel     the integer z-buffer to 0xFFFFFFFF and the counters to 0, on the stream: a captured step clears as an eager one does
//   align_scatter_kernel   one thread per raw pixel: its footprint's corners carried to the colour image, atomicMin of its depth over the covered pixels
//   align_finish_kernel    one thread per colour pixel: untouched -> 0, the rest to uint16, and the one-pixel cracks of the resampling closed
// The rule is stated in include/kpf.h.  Every floating-point operation is individually rounded and the only decision that depends on arrival order is an
// integer min: keypointfusion_amd/sensor.py::align_depth_host gives the same bits.
#include <math.h>

#include "kpf_common.h"

namespace {

constexpr int AL_MAXF = 32, AL_MAXPIX = 1 << 24, AL_MAXSPAN = 16, AL_CALIB = 21, AL_STATS = 5;
constexpr unsigned AL_EMPTY = 0xFFFFFFFFu;

struct AlignCalib {
  float k[AL_CALIB];  // fxd, fyd, u0d, v0d, fxc, fyc, u0c, v0c, R[9], t[3], unit_mm
};

// ---------------------------------------------------------------------------------------------------------------
// Launch 1: the clear.  n = F * Hc * Wc <= 2^29.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void align_clear_kernel(unsigned* __restrict__ zbuf, int n, int* __restrict__ stats, int nstats) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i < n) zbuf[i] = AL_EMPTY;
  if (i < nstats) stats[i] = 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 2: the scatter.  The calibrations travel in the kernel arguments (2688 bytes): the frame is uniform over the workgroup, so its row is read
// through scalar loads.  A wave's 64 raw pixels are 128 contiguous bytes of a row-major frame.
// ---------------------------------------------------------------------------------------------------------------
struct AlignScatterArgs {
  const unsigned short* raw;  // [F][Hd][Wd]
  unsigned* zbuf;             // [F][Hc][Wc]
  int* stats;                 // [F][5]
  int Hd, Wd, Hc, Wc;
  float max_span;
  AlignCalib cal[AL_MAXF];
};

// a point (pu, pv) of the depth image at depth z -> (u, v, Zc) in the colour camera
__device__ __forceinline__ void align_carry(const float* k, float pu, float pv, float z, float& u, float& v, float& Zc) {
#pragma clang fp contract(off)
  const float X = __fmul_rn(__fdiv_rn(__fsub_rn(pu, k[2]), k[0]), z), Y = __fmul_rn(__fdiv_rn(__fsub_rn(pv, k[3]), k[1]), z);
  const float Xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(k[8], X), __fmul_rn(k[9], Y)), __fmul_rn(k[10], z)), k[17]);
  const float Yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(k[11], X), __fmul_rn(k[12], Y)), __fmul_rn(k[13], z)), k[18]);
  Zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(k[14], X), __fmul_rn(k[15], Y)), __fmul_rn(k[16], z)), k[19]);
  u = __fadd_rn(__fdiv_rn(__fmul_rn(Xc, k[4]), Zc), k[6]);
  v = __fadd_rn(__fdiv_rn(__fmul_rn(Yc, k[5]), Zc), k[7]);
}

__device__ __forceinline__ int align_count(bool p) { return __popcll(__ballot(p)); }

__global__ __launch_bounds__(256) void align_scatter_kernel(AlignScatterArgs a) {
#pragma clang fp contract(off)
  __shared__ int cnt[3];  // valid, skipped, too_large of this workgroup
  const int t = threadIdx.x, frame = blockIdx.y, n = a.Hd * a.Wd;
  const int p = (int)blockIdx.x * 256 + t;
  if (t < 3) cnt[t] = 0;
  __syncthreads();
  const float* k = a.cal[frame].k;
  const unsigned short q = p < n ? a.raw[(long)frame * n + p] : (unsigned short)0;
  bool skipped = false, too_large = false;
  if (q != 0) {
    const int r = p / a.Wd, c = p - r * a.Wd;
    const float cf = (float)c, rf = (float)r, z = __fmul_rn((float)q, k[20]);
    float ua, va, za, ub, vb, zb, um, vm, zm;
    align_carry(k, __fsub_rn(cf, 0.5f), __fsub_rn(rf, 0.5f), z, ua, va, za);
    align_carry(k, __fadd_rn(cf, 0.5f), __fadd_rn(rf, 0.5f), z, ub, vb, zb);
    align_carry(k, cf, rf, z, um, vm, zm);
    const float d = rintf(zm);  // half to even
    const bool ok = za > 0.0f && zb > 0.0f && zm > 0.0f && d >= 1.0f && d <= 65535.0f && isfinite(ua) && isfinite(va) && isfinite(za) && isfinite(ub) &&
                    isfinite(vb) && isfinite(zb) && isfinite(um) && isfinite(vm) && isfinite(zm);
    skipped = !ok;
    if (ok) {
      // the colour pixels whose centres lie in [lo, hi) of the box of the two carried corners
      const float x0 = ceilf(fminf(ua, ub)), x1 = __fsub_rn(ceilf(fmaxf(ua, ub)), 1.0f);
      const float y0 = ceilf(fminf(va, vb)), y1 = __fsub_rn(ceilf(fmaxf(va, vb)), 1.0f);
      too_large = __fadd_rn(__fsub_rn(x1, x0), 1.0f) > a.max_span || __fadd_rn(__fsub_rn(y1, y0), 1.0f) > a.max_span;
      // clamped in float; converted only where the rectangle is not empty, so that every converted value lies on the grid
      const float X0 = fmaxf(x0, 0.0f), X1 = fminf(x1, (float)(a.Wc - 1)), Y0 = fmaxf(y0, 0.0f), Y1 = fminf(y1, (float)(a.Hc - 1));
      if (!too_large && X0 <= X1 && Y0 <= Y1) {
        const int ix0 = (int)X0, ix1 = (int)X1, iy0 = (int)Y0, iy1 = (int)Y1;
        const unsigned du = (unsigned)d;
        unsigned* zf = a.zbuf + (long)frame * a.Hc * a.Wc;
        for (int y = iy0; y <= iy1; ++y)
          for (int x = ix0; x <= ix1; ++x) atomicMin(&zf[(long)y * a.Wc + x], du);
      }
    }
  }
  // the counters: one LDS add per wave and one global add per workgroup, and none for a zero
  const int nv = align_count(q != 0), ns = align_count(skipped), nl = align_count(too_large);
  if ((t & 63) == 0) {
    if (nv) atomicAdd(&cnt[0], nv);
    if (ns) atomicAdd(&cnt[1], ns);
    if (nl) atomicAdd(&cnt[2], nl);
  }
  __syncthreads();
  if (t < 3 && cnt[t]) atomicAdd(&a.stats[frame * AL_STATS + t], cnt[t]);
}

// ---------------------------------------------------------------------------------------------------------------
// Launch 3: the finish.  Reads the z-buffer the scatter launch completed; the neighbours of the fill come from the same, unfilled, buffer.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void align_finish_kernel(const unsigned* __restrict__ zbuf, unsigned short* __restrict__ out, int* __restrict__ stats, int Hc,
                                                           int Wc, int fill) {
  __shared__ int cnt[2];  // covered, filled
  const int t = threadIdx.x, frame = blockIdx.y, n = Hc * Wc;
  const int p = (int)blockIdx.x * 256 + t;
  if (t < 2) cnt[t] = 0;
  __syncthreads();
  bool covered = false, filled = false;
  if (p < n) {
    const unsigned* zf = zbuf + (long)frame * n;
    unsigned v = zf[p];
    covered = v != AL_EMPTY;
    if (!covered) {
      v = 0;
      if (fill) {
        const int r = p / Wc, c = p - r * Wc;
        unsigned least = AL_EMPTY;
        int some = 0;
        if (r > 0 && zf[p - Wc] != AL_EMPTY) { least = min(least, zf[p - Wc]); ++some; }
        if (r < Hc - 1 && zf[p + Wc] != AL_EMPTY) { least = min(least, zf[p + Wc]); ++some; }
        if (c > 0 && zf[p - 1] != AL_EMPTY) { least = min(least, zf[p - 1]); ++some; }
        if (c < Wc - 1 && zf[p + 1] != AL_EMPTY) { least = min(least, zf[p + 1]); ++some; }
        filled = some >= 2;
        if (filled) v = least;
      }
    }
    out[(long)frame * n + p] = (unsigned short)v;
  }
  const int nc = align_count(covered), nf = align_count(filled);
  if ((t & 63) == 0) {
    if (nc) atomicAdd(&cnt[0], nc);
    if (nf) atomicAdd(&cnt[1], nf);
  }
  __syncthreads();
  if (t < 2 && cnt[t]) atomicAdd(&stats[frame * AL_STATS + 3 + t], cnt[t]);
}

}  // namespace

extern "C" int kpf_align_depth_u16(const unsigned short* depth_raw, int Hd, int Wd, const float* calib, int F, int Hc, int Wc, int max_span, int fill,
                                   unsigned* zbuf, unsigned short* depth_out, int* stats, void* stream) {
  const char* name = "kpf_align_depth_u16";
  KPF_REQUIRE(depth_raw && calib && zbuf && depth_out && stats, "%s: null pointer", name);
  KPF_REQUIRE(F >= 1 && F <= AL_MAXF && Hd >= 1 && Wd >= 1 && Hc >= 1 && Wc >= 1, "%s: bad shape F=%d Hd=%d Wd=%d Hc=%d Wc=%d (1 <= F <= %d; 1 <= Hd, Wd, Hc, Wc)",
              name, F, Hd, Wd, Hc, Wc, AL_MAXF);
  KPF_REQUIRE((long)Hd * Wd <= AL_MAXPIX && (long)Hc * Wc <= AL_MAXPIX, "%s: a frame of %d x %d or %d x %d holds more than 2^24 pixels", name, Hd, Wd, Hc, Wc);
  KPF_REQUIRE(max_span >= 1 && max_span <= AL_MAXSPAN, "%s: max_span=%d outside 1..%d", name, max_span, AL_MAXSPAN);
  KPF_REQUIRE(fill == 0 || fill == 1, "%s: fill=%d is neither 0 nor 1", name, fill);
  for (int f = 0; f < F; ++f) {
    const float* k = calib + (long)f * AL_CALIB;
    for (int i = 0; i < AL_CALIB; ++i) {
      const float v = k[i];
      KPF_REQUIRE(isfinite(v), "%s: calib[%d][%d]=%g is not finite", name, f, i, v);
    }
    KPF_REQUIRE(k[0] > 0.f && k[1] > 0.f && k[4] > 0.f && k[5] > 0.f, "%s: calib[%d] holds a focal length <= 0 (%g, %g, %g, %g)", name, f, k[0], k[1], k[4], k[5]);
    KPF_REQUIRE(k[20] > 0.f, "%s: calib[%d]: unit_mm=%g <= 0", name, f, k[20]);
  }
  {
    const uintptr_t in = reinterpret_cast<uintptr_t>(depth_raw), out = reinterpret_cast<uintptr_t>(depth_out);
    const uintptr_t in_bytes = (uintptr_t)F * Hd * Wd * 2, out_bytes = (uintptr_t)F * Hc * Wc * 2;
    KPF_REQUIRE(out + out_bytes <= in || in + in_bytes <= out, "%s: depth_out overlaps depth_raw", name);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nd = Hd * Wd, nc = Hc * Wc, nz = F * nc;  // <= 2^24, 2^24, 2^29
  hipLaunchKernelGGL(align_clear_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, s, zbuf, nz, stats, F * AL_STATS);
  AlignScatterArgs a;
  a.raw = depth_raw; a.zbuf = zbuf; a.stats = stats; a.Hd = Hd; a.Wd = Wd; a.Hc = Hc; a.Wc = Wc; a.max_span = (float)max_span;
  for (int i = 0; i < F * AL_CALIB; ++i) a.cal[i / AL_CALIB].k[i % AL_CALIB] = calib[i];
  for (int i = F * AL_CALIB; i < AL_MAXF * AL_CALIB; ++i) a.cal[i / AL_CALIB].k[i % AL_CALIB] = 0.f;  // the unused rows are zero
  hipLaunchKernelGGL(align_scatter_kernel, dim3((unsigned)((nd + 255) / 256), (unsigned)F), dim3(256), 0, s, a);
  hipLaunchKernelGGL(align_finish_kernel, dim3((unsigned)((nc + 255) / 256), (unsigned)F), dim3(256), 0, s, zbuf, depth_out, stats, Hc, Wc, fill);
  return kpf_check_launch(name);
}
