// The union-find, the pixel predicates and the key packing of the hand detector (csrc/kpf_detect.hip), as code that compiles for the host
// as well: tools/detect_uf_check.cpp drives these very functions sequentially, in shuffled orders, under the address and undefined-behaviour sanitizers.
//
// Invariant: L[x] <= x for every valid pixel x, always.  L starts as L[x] = x and is only ever written by fetch_min(&L[a], b) with b < a.
//   find   follows x <- L[x] while L[x] != x: x is a non-negative integer that strictly decreases, so the loop ends (at a pixel with L[x] == x).
//   union  each round takes the two roots a > b and does old = fetch_min(&L[a], b).  old == a: a was still a root and now hangs under b, done.  Otherwise
//          another union hung a under old < a first; L[a] is now min(old, b) and what remains is to join old and b, both < a: max(a, b) is a non-negative
//          integer that strictly decreases from round to round, so the loop ends.  No round waits for another thread.
// Every link goes from a pixel to a smaller one of its own component, so when all unions of a component are done its tree has one root, which is a member
// and not larger than any member: the component's smallest linear index, whatever the order of arrival.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KPF_UF_FN __host__ __device__ __forceinline__
constexpr int KPF_UF_WORKGROUP = __HIP_MEMORY_SCOPE_WORKGROUP, KPF_UF_AGENT = __HIP_MEMORY_SCOPE_AGENT;
#else
#define KPF_UF_FN inline
constexpr int KPF_UF_WORKGROUP = 0, KPF_UF_AGENT = 1;
#endif

// relaxed atomics of the given scope on the device; plain accesses on the host, where the emulation is sequential
template <int SCOPE>
KPF_UF_FN int kpf_uf_load(int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
#else
  return *p;
#endif
}
template <int SCOPE>
KPF_UF_FN int kpf_uf_fetch_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE);
#else
  const int old = *p;
  if (v < old) *p = v;
  return old;
#endif
}

template <int SCOPE>
KPF_UF_FN int kpf_uf_find(int* L, int x) {
  int p = kpf_uf_load<SCOPE>(L + x);
  while (p != x) {  // p < x
    x = p;
    p = kpf_uf_load<SCOPE>(L + x);
  }
  return x;
}

template <int SCOPE>
KPF_UF_FN void kpf_uf_union(int* L, int a, int b) {
  for (;;) {
    a = kpf_uf_find<SCOPE>(L, a);
    b = kpf_uf_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = kpf_uf_fetch_min<SCOPE>(L + a, b);  // a > b
    if (old == a) return;
    a = old;  // old < a
  }
}

// step 1 of the rule: near <= d <= far
KPF_UF_FN bool kpf_detect_valid(int d, int near, int far) { return d >= near && d <= far; }
// step 2: two 4-neighbours are joined when both are valid and |da - db| <= step_mm
KPF_UF_FN bool kpf_detect_joined(int da, int db, int near, int far, int step_mm) {
  const int diff = da > db ? da - db : db - da;
  return kpf_detect_valid(da, near, far) && kpf_detect_valid(db, near, far) && diff <= step_mm;
}

// step 6: candidates are ranked by (z_min, label) ascending = by this key; z_min <= 65535, 0 <= label < 2^24
constexpr unsigned long long KPF_DETECT_NOKEY = ~0ull;
KPF_UF_FN unsigned long long kpf_detect_key(int z_min, int label) { return ((unsigned long long)(unsigned)z_min << 32) | (unsigned long long)(unsigned)label; }
KPF_UF_FN int kpf_detect_key_zmin(unsigned long long key) { return (int)(key >> 32); }
KPF_UF_FN int kpf_detect_key_label(unsigned long long key) { return (int)(key & 0xffffffffull); }
