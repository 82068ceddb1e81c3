// Envelope-reducing variable order of a block-compact Hessian (thx_hblock_order, host only) and the block-list gather that moves
// the linearization's blocks into a layout built on that order (thx_hblocks_permute).  DESIGN.md 4.1.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "common.cuh"

namespace thx {
namespace {

// undirected variable graph of the off-diagonal blocks, neighbours ascending and unique
struct VarGraph {
  int32_t n = 0;
  std::vector<int32_t> ptr, adj;
  int32_t deg(int32_t v) const { return ptr[v + 1] - ptr[v]; }
};

bool build_graph(int32_t nvars, int32_t nblocks, const int32_t* blocks, VarGraph& g) {
  std::vector<std::pair<int32_t, int32_t>> e;
  e.reserve(2 * (size_t)nblocks);
  for (int32_t k = 0; k < nblocks; ++k) {
    const int32_t p = blocks[2 * k], q = blocks[2 * k + 1];
    if (p < 0 || p >= nvars || q < 0 || q > p) return false;
    if (q < p) {
      e.emplace_back(p, q);
      e.emplace_back(q, p);
    }
  }
  std::sort(e.begin(), e.end());
  e.erase(std::unique(e.begin(), e.end()), e.end());
  g.n = nvars;
  g.ptr.assign(nvars + 1, 0);
  g.adj.resize(e.size());
  for (auto& x : e) ++g.ptr[x.first + 1];
  for (int32_t v = 0; v < nvars; ++v) g.ptr[v + 1] += g.ptr[v];
  for (size_t k = 0; k < e.size(); ++k) g.adj[k] = e[k].second;   // (sorted by (first, second): already in CSR order)
  return true;
}

// sum over scalar rows r of (r - first[r])^2 with ``order[k]`` = the variable at position k: row bd k + i begins at column
// bd * (the smallest position among variable order[k] and its neighbours) -- the envelope of P H P^T, which its factor fills
// and never leaves
int64_t envelope_score(const VarGraph& g, int32_t bd, const std::vector<int32_t>& order, std::vector<int32_t>& pos) {
  for (int32_t k = 0; k < g.n; ++k) pos[order[k]] = k;
  int64_t s = 0;
  for (int32_t k = 0; k < g.n; ++k) {
    const int32_t v = order[k];
    int32_t f = k;
    for (int32_t a = g.ptr[v]; a < g.ptr[v + 1]; ++a) f = std::min(f, pos[g.adj[a]]);
    const int64_t w = (int64_t)bd * (k - f);
    for (int32_t i = 0; i < bd; ++i) s += (w + i) * (w + i);
  }
  return s;
}

// breadth-first levels from ``s`` inside its component: the node of the last level with the lowest degree (lowest index on a
// tie) and the number of levels
std::pair<int32_t, int32_t> bfs_far(const VarGraph& g, int32_t s, std::vector<int32_t>& level, std::vector<int32_t>& queue) {
  std::fill(level.begin(), level.end(), -1);
  queue.clear();
  queue.push_back(s);
  level[s] = 0;
  for (size_t h = 0; h < queue.size(); ++h) {
    const int32_t v = queue[h];
    for (int32_t a = g.ptr[v]; a < g.ptr[v + 1]; ++a)
      if (level[g.adj[a]] < 0) {
        level[g.adj[a]] = level[v] + 1;
        queue.push_back(g.adj[a]);
      }
  }
  const int32_t last = level[queue.back()];
  int32_t best = queue.back();
  for (int32_t v : queue)
    if (level[v] == last && (g.deg(v) < g.deg(best) || (g.deg(v) == g.deg(best) && v < best))) best = v;
  return {best, last + 1};
}

// the two ends of a pseudo-diameter of the component of ``s`` (George-Liu: walk to a far node until the depth stops growing)
std::pair<int32_t, int32_t> pseudo_peripheral(const VarGraph& g, int32_t s, std::vector<int32_t>& level, std::vector<int32_t>& queue) {
  int32_t u = s;
  auto fu = bfs_far(g, u, level, queue);
  for (int it = 0; it < 8; ++it) {
    const int32_t v = fu.first;
    const auto fv = bfs_far(g, v, level, queue);
    if (fv.second <= fu.second) return {u, v};
    u = v;
    fu = fv;
  }
  return {u, fu.first};
}

// Cuthill-McKee from ``start`` (neighbours by ascending degree, then index); further components start at their unvisited
// variable of lowest index
void cuthill_mckee(const VarGraph& g, int32_t start, std::vector<int32_t>& order) {
  std::vector<char> seen(g.n, 0);
  std::vector<int32_t> nb;
  order.clear();
  int32_t next_free = 0;
  for (int32_t s = start; (int32_t)order.size() < g.n;) {
    size_t h = order.size();
    order.push_back(s);
    seen[s] = 1;
    for (; h < order.size(); ++h) {
      const int32_t v = order[h];
      nb.clear();
      for (int32_t a = g.ptr[v]; a < g.ptr[v + 1]; ++a)
        if (!seen[g.adj[a]]) nb.push_back(g.adj[a]);
      std::sort(nb.begin(), nb.end(), [&](int32_t x, int32_t y) { return g.deg(x) != g.deg(y) ? g.deg(x) < g.deg(y) : x < y; });
      for (int32_t w : nb) {
        seen[w] = 1;
        order.push_back(w);
      }
    }
    while (next_free < g.n && seen[next_free]) ++next_free;
    s = next_free;
  }
}

// Greedy minimum-front-growth order (King): the next variable is the one of the front -- the unnumbered neighbours of the numbered
// variables -- whose numbering adds the fewest new variables to the front; ties go to the variable that has waited in the front
// longest, then to the lowest index.  An empty front (start, a new component) takes ``start`` / the unnumbered variable of lowest
// degree, lowest index.
void king(const VarGraph& g, int32_t start, std::vector<int32_t>& order) {
  constexpr int32_t NUMBERED = -2, OUT = -1;
  std::vector<int32_t> since(g.n, OUT);   // OUT, NUMBERED, or the step at which the variable entered the front
  std::vector<int32_t> front;
  order.clear();
  int32_t pick = start;
  for (int32_t step = 0; step < g.n; ++step) {
    if (pick < 0) {
      int64_t bestg = INT64_MAX;
      for (int32_t v : front) {
        int32_t grow = 0;
        for (int32_t a = g.ptr[v]; a < g.ptr[v + 1]; ++a) grow += since[g.adj[a]] == OUT;
        const int64_t key = ((int64_t)grow << 32) | since[v];
        if (key < bestg || (key == bestg && v < pick)) {
          bestg = key;
          pick = v;
        }
      }
      if (pick < 0)   // a new component
        for (int32_t v = 0; v < g.n; ++v)
          if (since[v] == OUT && (pick < 0 || g.deg(v) < g.deg(pick))) pick = v;
    }
    if (since[pick] >= 0) front.erase(std::find(front.begin(), front.end(), pick));
    since[pick] = NUMBERED;
    order.push_back(pick);
    for (int32_t a = g.ptr[pick]; a < g.ptr[pick + 1]; ++a)
      if (since[g.adj[a]] == OUT) {
        since[g.adj[a]] = step;
        front.push_back(g.adj[a]);
      }
    pick = -1;
  }
}

}  // namespace

template <typename T>
__global__ void hblocks_permute_kernel(const T* __restrict__ src, int64_t sstride, T* __restrict__ dst, int64_t dstride,
                                       const int32_t* __restrict__ map, int nelems, int bd) {
  const int b = blockIdx.y, idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nelems) return;
  const int bb = bd * bd, k = idx / bb, e = idx % bb;
  const int m = map[k];
  const int se = (m & 1) ? (e % bd) * bd + e / bd : e;
  dst[(int64_t)b * dstride + idx] = src[(int64_t)b * sstride + (int64_t)(m >> 1) * bb + se];
}

// (bd^2 a multiple of four, strides too: four consecutive elements of a destination block per thread -- one 16-byte (fp32) /
//  32-byte (fp64) store, and one such load where the block is not transposed)
template <typename T>
__global__ void hblocks_permute4_kernel(const T* __restrict__ src, int64_t sstride, T* __restrict__ dst, int64_t dstride,
                                        const int32_t* __restrict__ map, int nquads, int bd) {
  typedef T T4 __attribute__((ext_vector_type(4)));
  const int b = blockIdx.y, q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nquads) return;
  const int bb = bd * bd, qb = bb / 4, k = q / qb, e0 = 4 * (q % qb);
  const int m = map[k];
  const T* from = src + (int64_t)b * sstride + (int64_t)(m >> 1) * bb;
  T4 v;
  if (m & 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = from[((e0 + i) % bd) * bd + (e0 + i) / bd];
  } else {
    v = *reinterpret_cast<const T4*>(from + e0);
  }
  *reinterpret_cast<T4*>(dst + (int64_t)b * dstride + (int64_t)k * bb + e0) = v;
}

// the lower triangle of P H P^T from the lower triangle of H: Hp[i][j] = H[max(idx[i], idx[j])][min(idx[i], idx[j])], j <= i < n
template <typename T>
__global__ void frame_permute_kernel(const T* __restrict__ H, int64_t ld, T* __restrict__ Hp, int64_t ldp,
                                     const int32_t* __restrict__ idx, int n) {
  const int b = blockIdx.z, i = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > i) return;
  const int a = idx[i], c = idx[j];
  Hp[(int64_t)b * ldp * ldp + (int64_t)i * ldp + j] = H[(int64_t)b * ld * ld + (int64_t)max(a, c) * ld + min(a, c)];
}

}  // namespace thx

using namespace thx;

int thx_hblock_order(int32_t nvars, int32_t bd, int32_t nblocks, const int32_t* blocks, int32_t* perm_out, int64_t* score_out) {
  if (nvars <= 0 || bd <= 0 || nblocks < 0 || (nblocks > 0 && !blocks) || !perm_out) return fail("thx_hblock_order: bad arguments");
  if ((int64_t)nvars * bd > (int64_t)1 << 20) return fail("thx_hblock_order: matrix too large");   // (the score stays inside int64)
  VarGraph g;
  if (!build_graph(nvars, nblocks, blocks, g)) return fail("thx_hblock_order: a block outside tril(H)");
  std::vector<int32_t> best(nvars), cand, rev, pos(nvars), level(nvars), queue;
  for (int32_t v = 0; v < nvars; ++v) best[v] = v;
  const int64_t natural = envelope_score(g, bd, best, pos);
  int64_t best_score = natural;
  auto offer = [&](const std::vector<int32_t>& o) {   // (strictly better only: insertion order keeps every tie)
    const int64_t s = envelope_score(g, bd, o, pos);
    if (s < best_score) {
      best_score = s;
      best = o;
    }
  };
  auto offer_both = [&](const std::vector<int32_t>& o) {
    offer(o);
    rev.assign(o.rbegin(), o.rend());
    offer(rev);
  };
  // start nodes: both ends of a pseudo-diameter, the first and the last variable, the four variables of lowest degree
  std::vector<int32_t> starts;
  const auto ends = pseudo_peripheral(g, 0, level, queue);
  starts = {ends.first, ends.second, 0, nvars - 1};
  {
    std::vector<int32_t> by_deg(nvars);
    for (int32_t v = 0; v < nvars; ++v) by_deg[v] = v;
    const int32_t take = std::min<int32_t>(4, nvars);
    std::partial_sort(by_deg.begin(), by_deg.begin() + take, by_deg.end(),
                      [&](int32_t x, int32_t y) { return g.deg(x) != g.deg(y) ? g.deg(x) < g.deg(y) : x < y; });
    starts.insert(starts.end(), by_deg.begin(), by_deg.begin() + take);
  }
  {
    std::vector<int32_t> uniq;
    for (int32_t s : starts)
      if (std::find(uniq.begin(), uniq.end(), s) == uniq.end()) uniq.push_back(s);
    starts.swap(uniq);
  }
  cuthill_mckee(g, ends.first, cand);   // Cuthill-McKee and its reverse
  offer_both(cand);
  cuthill_mckee(g, ends.second, cand);
  offer_both(cand);
  if (nvars <= 16384)   // (the greedy order is quadratic in the front)
    for (int32_t s : starts) {
      king(g, s, cand);
      offer_both(cand);
    }
  std::copy(best.begin(), best.end(), perm_out);
  if (score_out) {
    score_out[0] = best_score;
    score_out[1] = natural;
  }
  return 0;
}

int thx_hblocks_permute(const void* src, int64_t sstride, void* dst, int64_t dstride, const int32_t* map, int32_t nblocks, int32_t bd,
                        int32_t B, int dtype, void* stream) {
  if (!src || !dst || !map || nblocks <= 0 || bd <= 0 || B <= 0 || B > 65535 || src == dst) return fail("thx_hblocks_permute: bad args");
  const int64_t nelems = (int64_t)nblocks * bd * bd;
  if (nelems > INT32_MAX || sstride < nelems || dstride < nelems) return fail("thx_hblocks_permute: the lists are shorter than nblocks blocks");
  const size_t vec = dtype == THX_F64 ? 32 : 16;
  if ((bd * bd) % 4 == 0 && sstride % 4 == 0 && dstride % 4 == 0 && reinterpret_cast<uintptr_t>(src) % vec == 0 &&
      reinterpret_cast<uintptr_t>(dst) % vec == 0) {
    const int nquads = (int)(nelems / 4);
    dim3 grid4((unsigned)((nquads + 255) / 256), B);
    THX_DISPATCH(dtype,
                 hipLaunchKernelGGL(hblocks_permute4_kernel<float>, grid4, dim3(256), 0, as_stream(stream), (const float*)src, sstride,
                                    (float*)dst, dstride, map, nquads, bd),
                 hipLaunchKernelGGL(hblocks_permute4_kernel<double>, grid4, dim3(256), 0, as_stream(stream), (const double*)src,
                                    sstride, (double*)dst, dstride, map, nquads, bd));
    return check_launch("thx_hblocks_permute");
  }
  dim3 grid((unsigned)((nelems + 255) / 256), B), block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(hblocks_permute_kernel<float>, grid, block, 0, as_stream(stream), (const float*)src, sstride,
                                  (float*)dst, dstride, map, (int)nelems, bd),
               hipLaunchKernelGGL(hblocks_permute_kernel<double>, grid, block, 0, as_stream(stream), (const double*)src, sstride,
                                  (double*)dst, dstride, map, (int)nelems, bd));
  return check_launch("thx_hblocks_permute");
}

int thx_frame_permute(const void* H, int64_t ld, void* Hp, int64_t ldp, const int32_t* idx, int32_t n, int32_t B, int dtype,
                      void* stream) {
  if (!H || !Hp || !idx || n <= 0 || n > 65535 || B <= 0 || B > 65535 || ld < n || ldp < n || H == Hp)
    return fail("thx_frame_permute: bad args");
  dim3 grid((n + 255) / 256, n, B), block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(frame_permute_kernel<float>, grid, block, 0, as_stream(stream), (const float*)H, ld, (float*)Hp,
                                  ldp, idx, n),
               hipLaunchKernelGGL(frame_permute_kernel<double>, grid, block, 0, as_stream(stream), (const double*)H, ld,
                                  (double*)Hp, ldp, idx, n));
  return check_launch("thx_frame_permute");
}
