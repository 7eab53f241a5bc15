// The reference loader's box rule (dataloader/loader.py get_bbox with expansion e in float32, every operation rounded; process_bbox with expansion 1 and
// aspect ratio 1 in float64) = tracking.next_bbox, the host yardstick, bit for bit.  The one definition behind kpf_track_step_f32 (the extent of the joints)
// and kpf_detect_hands_u16 (the extent of a near slab): their boxes are the same arithmetic.  Contraction is off inside every function (the Makefile's
// -ffp-contract=on would fuse the float32 steps of the rule, which numpy rounds one by one).
#pragma once

// get_bbox along one axis in float32: (corner, size) of the extent [lo, hi] grown by e about its middle
__device__ __forceinline__ void kpf_box_expand(float lo, float hi, float e, float& corner, float& size) {
#pragma clang fp contract(off)
  const float c = (lo + hi) / 2.0f;
  const float w = (hi - lo) * e;
  const float a = c - 0.5f * w;
  const float b = c + 0.5f * w;
  corner = a;
  size = b - a;
}

// numpy's reductions over a pair: np.max((a, b)) = a if a >= b else b, np.min((a, b)) = a if a <= b else b (no NaN reaches them here)
__device__ __forceinline__ double kpf_box_max2(double a, double b) { return a >= b ? a : b; }
__device__ __forceinline__ double kpf_box_min2(double a, double b) { return a <= b ? a : b; }

// the extent [ulo, uhi] x [vlo, vhi] in float32 frame pixels -> box (x, y, w, h) in float64; false: the rule gives no box (next_bbox's None), box untouched
__device__ __forceinline__ bool kpf_next_box(float ulo, float uhi, float vlo, float vhi, float expansion, int frame_w, int frame_h, double* box) {
#pragma clang fp contract(off)
  float bx, bw, by, bh;
  kpf_box_expand(ulo, uhi, expansion, bx, bw);
  kpf_box_expand(vlo, vhi, expansion, by, bh);
  // process_bbox(expansion 1, aspect ratio 1) in float64 on the four float32 values
  const double X1 = kpf_box_max2(0.0, (double)bx), Y1 = kpf_box_max2(0.0, (double)by);
  const double X2 = kpf_box_min2((double)(frame_w - 1), X1 + kpf_box_max2(0.0, (double)bw - 1.0));
  const double Y2 = kpf_box_min2((double)(frame_h - 1), Y1 + kpf_box_max2(0.0, (double)bh - 1.0));
  if (!((double)bw * (double)bh > 0.0 && X2 >= X1 && Y2 >= Y1)) return false;
  double w = X2 - X1, h = Y2 - Y1;
  const double cx = X1 + w / 2.0, cy = Y1 + h / 2.0;
  if (w > h)
    h = w;
  else if (w < h)
    w = h;
  box[0] = cx - w / 2.0;
  box[1] = cy - h / 2.0;
  box[2] = w;
  box[3] = h;
  return true;
}
