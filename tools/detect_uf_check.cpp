// Host check of keypointfusion_amd/csrc/kpf_detect_uf.h, the union-find, pixel predicates and key packing of the hand detector: the very
// functions the kernels call, driven sequentially in shuffled orders over scene files, the labels compared with the numpy restatement's.  A stand-alone
// program, meant to be built with the sanitizers (tests/test_detect_host.py does both):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I keypointfusion_amd/csrc tools/detect_uf_check.cpp -o detect_uf_check
//   ./detect_uf_check scene.bin [...]
//
// A scene file is int32 {H, W, near, far, step_mm}, uint16 depth[H * W], int32 labels[H * W] (the expected labels, -1 where invalid).  Per scene and order
// (row-major, reversed, 6 shuffles) it emulates the kernels' three labelling launches -- 32 x 32 tiles resolved in a local array, seam unions on the frame's
// parents, flatten -- and one plain pass of every union on the frame's parents.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#include "kpf_detect_uf.h"

namespace {

constexpr int TILE = 32;

struct Scene {
  int H = 0, W = 0, near = 0, far = 0, step = 0;
  std::vector<uint16_t> depth;
  std::vector<int32_t> labels;
};

bool read_scene(const char* path, Scene& s) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[5];
  bool ok = fread(h, sizeof(int32_t), 5, f) == 5 && h[0] >= 1 && h[1] >= 1 && (long)h[0] * h[1] <= (1 << 24);
  if (ok) {
    s.H = h[0]; s.W = h[1]; s.near = h[2]; s.far = h[3]; s.step = h[4];
    const size_t n = (size_t)s.H * s.W;
    s.depth.resize(n);
    s.labels.resize(n);
    ok = fread(s.depth.data(), sizeof(uint16_t), n, f) == n && fread(s.labels.data(), sizeof(int32_t), n, f) == n;
  }
  fclose(f);
  return ok;
}

void order_edges(std::vector<std::pair<int, int>>& e, int order) {
  if (order == 1) std::reverse(e.begin(), e.end());
  if (order >= 2) {
    std::mt19937 g((unsigned)order);
    std::shuffle(e.begin(), e.end(), g);
  }
}

int compare(const Scene& s, std::vector<int>& parent, const char* what, int order, const char* path) {
  const int n = s.H * s.W;
  for (int p = 0; p < n; ++p) {
    const bool valid = kpf_detect_valid(s.depth[p], s.near, s.far);
    const int got = valid ? kpf_uf_find<KPF_UF_AGENT>(parent.data(), p) : -1;
    if (got != s.labels[p]) {
      fprintf(stderr, "%s: %s, order %d: pixel %d has label %d, expected %d\n", path, what, order, p, got, s.labels[p]);
      return 1;
    }
  }
  return 0;
}

// the three labelling launches of kpf_detect.hip
int tiled(const Scene& s, int order, const char* path) {
  const int H = s.H, W = s.W;
  std::vector<int> parent((size_t)H * W, -1);
  for (int y0 = 0; y0 < H; y0 += TILE)
    for (int x0 = 0; x0 < W; x0 += TILE) {
      int lab[TILE * TILE];
      int dd[TILE * TILE];
      bool ok[TILE * TILE];
      for (int l = 0; l < TILE * TILE; ++l) {
        const int y = y0 + l / TILE, x = x0 + l % TILE;
        const bool in = y < H && x < W;
        dd[l] = in ? s.depth[(size_t)y * W + x] : 0;
        ok[l] = in && kpf_detect_valid(dd[l], s.near, s.far);
        lab[l] = l;
      }
      std::vector<std::pair<int, int>> e;
      for (int l = 0; l < TILE * TILE; ++l) {
        if (!ok[l]) continue;
        if (l % TILE > 0 && kpf_detect_joined(dd[l], dd[l - 1], s.near, s.far, s.step)) e.push_back({l, l - 1});
        if (l >= TILE && kpf_detect_joined(dd[l], dd[l - TILE], s.near, s.far, s.step)) e.push_back({l, l - TILE});
      }
      order_edges(e, order);
      for (const auto& ab : e) kpf_uf_union<KPF_UF_WORKGROUP>(lab, ab.first, ab.second);
      for (int l = 0; l < TILE * TILE; ++l) {
        const int y = y0 + l / TILE, x = x0 + l % TILE;
        if (!(y < H && x < W) || !ok[l]) continue;
        const int r = kpf_uf_find<KPF_UF_WORKGROUP>(lab, l);
        parent[(size_t)y * W + x] = (y0 + r / TILE) * W + x0 + r % TILE;
      }
    }
  std::vector<std::pair<int, int>> e;
  for (int p = 0; p < H * W; ++p) {
    const int y = p / W, x = p - y * W;
    if (x > 0 && x % TILE == 0 && kpf_detect_joined(s.depth[p], s.depth[p - 1], s.near, s.far, s.step)) e.push_back({p, p - 1});
    if (y > 0 && y % TILE == 0 && kpf_detect_joined(s.depth[p], s.depth[p - W], s.near, s.far, s.step)) e.push_back({p, p - W});
  }
  order_edges(e, order);
  for (const auto& ab : e) kpf_uf_union<KPF_UF_AGENT>(parent.data(), ab.first, ab.second);
  return compare(s, parent, "tiles + seams", order, path);
}

// every union on the frame's parents, no tiles
int plain(const Scene& s, int order, const char* path) {
  const int H = s.H, W = s.W;
  std::vector<int> parent((size_t)H * W);
  std::iota(parent.begin(), parent.end(), 0);
  std::vector<std::pair<int, int>> e;
  for (int p = 0; p < H * W; ++p) {
    const int y = p / W, x = p - y * W;
    if (x > 0 && kpf_detect_joined(s.depth[p], s.depth[p - 1], s.near, s.far, s.step)) e.push_back({p, p - 1});
    if (y > 0 && kpf_detect_joined(s.depth[p], s.depth[p - W], s.near, s.far, s.step)) e.push_back({p, p - W});
  }
  order_edges(e, order);
  for (const auto& ab : e) kpf_uf_union<KPF_UF_AGENT>(parent.data(), ab.first, ab.second);
  return compare(s, parent, "plain", order, path);
}

int keys() {
  int bad = 0;
  const int z[4] = {0, 171, 1500, 65535}, l[4] = {0, 1, 65536, (1 << 24) - 1};
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      const unsigned long long a = kpf_detect_key(z[i / 4], l[i % 4]), b = kpf_detect_key(z[j / 4], l[j % 4]);
      const bool less = z[i / 4] < z[j / 4] || (z[i / 4] == z[j / 4] && l[i % 4] < l[j % 4]);
      bad += (a < b) != less;
      bad += kpf_detect_key_zmin(a) != z[i / 4] || kpf_detect_key_label(a) != l[i % 4] || a == KPF_DETECT_NOKEY;
    }
  if (bad) fprintf(stderr, "key packing: %d mismatches\n", bad);
  return bad != 0;
}

}  // namespace

int main(int argc, char** argv) {
  int bad = keys();
  for (int i = 1; i < argc; ++i) {
    Scene s;
    if (!read_scene(argv[i], s)) {
      fprintf(stderr, "%s: not a scene file\n", argv[i]);
      return 2;
    }
    for (int order = 0; order < 8; ++order) bad += tiled(s, order, argv[i]) + plain(s, order, argv[i]);
  }
  printf("detect_uf_check: %d scene file(s), %s\n", argc - 1, bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}
