// Connected components by a tiled union-find, stated once for canny.hip (hysteresis), slic.hip (connectivity) and instances.hip
// (DESIGN.md 10j).  The kernels stay in those files with their grids and side effects; these are the device-inline pieces they share:
//
//   uf_find / uf_union   lock-free union-find on an int array of parents
//   cc_run_parent        label tiles, first half: every member starts out pointing at the first pixel of its run in the tile row
//   cc_tile_unions       label tiles, second half: the unions of one pixel with the row above, those left out that say nothing new
//   cc_tile_root         label tiles, last: a tile entry's root as an index of the batch
//   cc_join_borders      join tiles: the same unions across the tile borders, on the global parents
//   cc_flatten           flatten: one pixel finds its root and points at it
// (the scan and rank launches that follow use block_chunk_prefix and block_rank of label_inl.h)
//
// CONN is 4 or 8, T the tile side.  Two member pixels a, b that touch are LINKED when same(a, b): always for Canny and the instances
// (cc_all), on equal labels for SLIC: `same` is an equivalence.  A union with the pixel above or to the left is left out only where
// the three links that replace it have been checked, none assumed; with cc_all the rules fold to the ones instances.hip was first
// written with.  tests/cc_rule_ref.py restates them and tests/test_cc_rule.py holds them to a flood fill on every small input.
#pragma once
#include <hip/hip_runtime.h>

// An entry is its own index at a root, a smaller index of its component elsewhere.  SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP on LDS,
// __HIP_MEMORY_SCOPE_AGENT on global memory.
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* L, int x) {
  for (;;) {
    const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
    if (p == x) return x;
    x = p;
  }
}
// joins the components of a and b.  The larger root is pointed at the smaller with atomicMin: parents only ever decrease, so there
// are no cycles and a component's root is its smallest index whatever the order the unions ran in.  When another thread linked that
// root first (the old value is not the root itself) its new parent still has to meet b: once more from there
template <int SCOPE>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(L, a); b = uf_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;
    a = old;
  }
}

struct cc_all {
  template <class I> __device__ bool operator()(I, I) const { return true; }
};

// Tile entry l = tid + k NT of a block of NT threads, called by every thread: a row of the tile is half a wave, so one ballot of the
// members (and one of the members cut off from their left neighbour by `same`) gives a member the first pixel of its run -- a maximal
// stretch of members each linked to the one on its left -- as its first parent.  -> that entry, -1 for a non-member.
template <int T, int NT, class Same>
__device__ __forceinline__ int cc_run_parent(int l, bool member, Same same) {
  static_assert(T == 32 && NT % 64 == 0, "a tile row is half a wave, and l = tid + k NT keeps a thread's lane: whole waves");
  const unsigned lx = l & 31, half = l & 32;
  const unsigned row = (unsigned)(__ballot(member) >> half);
  const bool cut = member && lx > 0 && (row >> (lx - 1) & 1u) && !same(l, l - 1);
  const unsigned linked = row & (row << 1) & ~(unsigned)(__ballot(cut) >> half);      // bit x: x is linked to x - 1
  const unsigned starts = ~linked & ((2u << lx) - 1u);                               // the run starts at or before lx; bit 0 is one
  return member ? l - (int)lx + 31 - __clz((int)starts) : -1;
}

// The runs of one row meet the row above: the unions of tile entry l (lab[] >= 0 at a member, from cc_run_parent) after a barrier.
// A union is left out where the neighbours' unions say the same.  With the pixel above: when the pixel to the left (same run) is
// linked to the one above it and that one to the pixel above -- three links, each checked.  With a diagonal pixel: when p is linked
// to the pixel above (`same` is an equivalence: the pixel above is then linked to the diagonal one, in its own row's runs) or,
// for the upper left, through the pixel to the left.
template <int CONN, int T, class Same>
__device__ __forceinline__ void cc_tile_unions(int* lab, int l, Same same) {
  if (lab[l] < 0 || l < T) return;                                // (a member's entry never goes negative)
  constexpr int SC = __HIP_MEMORY_SCOPE_WORKGROUP;
  const int lx = l % T;
  const bool m_up = lab[l - T] >= 0, m_left = lx > 0 && lab[l - 1] >= 0, m_nw = lx > 0 && lab[l - T - 1] >= 0;      // members among the neighbours
  const bool by_left = m_left && m_nw && same(l, l - 1) && same(l - 1, l - T - 1);      // joined with the upper left pixel through the left one
  if (m_up && same(l, l - T)) {
    if (!(by_left && same(l - T - 1, l - T))) uf_union<SC>(lab, l, l - T);
  } else if (CONN == 8) {
    if (m_nw && !by_left && same(l, l - T - 1)) uf_union<SC>(lab, l, l - T - 1);
    if (lx < T - 1 && lab[l - T + 1] >= 0 && same(l, l - T + 1)) uf_union<SC>(lab, l, l - T + 1);
  }
}

// The root of member entry l of the tile at (y0, x0) as an index of the batch (base: the image's first pixel), after a barrier: no
// entry changes any more.  Row-major order inside the tile is the order of the batch index, so the tile's root is its smallest.
template <int T>
__device__ __forceinline__ int cc_tile_root(int* lab, int l, size_t base, int y0, int x0, int W) {
  const int q = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l);
  return (int)(base + (size_t)(y0 + q / T) * W + (x0 + q % T));
}

// Pixel p of a batch of H x W images whose tiles are labelled in par[]: its unions across the tile borders, agent scope.  member(q)
// and same(a, b) read whatever the caller's membership lives in.  A neighbour is a pixel of the same image, never the next image's
// first row or the row's other end.  Left out by cc_tile_unions' rule: across a column border when the pixel above (same tile) is
// linked to p and to the one on its left, and that one to the pixel on p's left; across a row border likewise with left and above
// exchanged; a tile's corner pixel leaves out neither.  Diagonally: as in the tile.
template <int CONN, int T, class Member, class Same>
__device__ __forceinline__ void cc_join_borders(int* par, long long p, int H, int W, Member member, Same same) {
  const int q = (int)(p % ((long long)H * W)), y = q / W, x = q - y * W;
  const int ty = y % T, tx = x % T;
  if (ty != 0 && tx != 0 && (CONN == 4 || tx != T - 1)) return;
  if (!member(p)) return;
  constexpr int SC = __HIP_MEMORY_SCOPE_AGENT;
  const int i = (int)p;
  const bool m_left = x > 0 && member(p - 1), m_up = y > 0 && member(p - W), m_nw = x > 0 && y > 0 && member(p - W - 1);
  const bool left = m_left && same(p, p - 1), up = m_up && same(p, p - W);
  const bool nw_left = m_nw && m_left && same(p - W - 1, p - 1), nw_up = m_nw && m_up && same(p - W - 1, p - W);
  if (tx == 0 && left && !(ty != 0 && up && nw_up && nw_left)) uf_union<SC>(par, i, i - 1);
  if (ty == 0 && up && !(tx != 0 && left && nw_left && nw_up)) uf_union<SC>(par, i, i - W);
  if (CONN == 8 && !up) {
    if ((ty == 0 || tx == 0) && m_nw && !(left && nw_left) && same(p, p - W - 1)) uf_union<SC>(par, i, i - W - 1);
    if ((ty == 0 || tx == T - 1) && y > 0 && x < W - 1 && member(p - W + 1) && same(p, p - W + 1)) uf_union<SC>(par, i, i - W + 1);
  }
}

// Member p finds its root and points at it.  Other threads shorten chains meanwhile: an entry read here is the old parent or the
// root, both lead to the root.  -> the root
__device__ __forceinline__ int cc_flatten(int* par, long long p) {
  const int r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(par, (int)p);
  if (r != (int)p) __hip_atomic_store(par + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return r;
}
