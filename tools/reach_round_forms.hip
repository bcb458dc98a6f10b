// reach_round_forms.hip -- a stand-alone measurement (its own main; not part of the library): the reach field's rounds in the two
// forms DESIGN.md 3.19 weighs.  The COMPACTED LIST is what reach.hip ships (this file includes it and calls its launchers): a
// round launches one workgroup per active tile.  The EARLY-EXIT GRID launches one workgroup per tile of the grid every round; a
// workgroup whose tile's flag is clear leaves at once, and a mark sets a flag and adds to the round's count without a list.  Both
// run the same tile relaxation (hsk_reach_point.h), are driven by the same host loop -- a round, then the read-back of the number of
// tiles marked -- and must give the same field.  Input: an N^3 grid, passable but for a hashed fraction of the voxels, one seed at
// the centre: the field fills the grid, the large case of tools/reach_bench.py.  Prints the rounds, the tiles relaxed and ms.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I housescan_amd/csrc tools/reach_round_forms.hip -o reach_round_forms && ./reach_round_forms [N] [blocked per million]
#include "../housescan_amd/csrc/reach.hip"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(call)                                                                      \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) {                                                              \
      fprintf(stderr, "%s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

// clearance values: 0 (an obstacle) at a hashed fraction of the voxels, far elsewhere
__global__ __launch_bounds__(256) void k_fill(unsigned* __restrict__ d2, unsigned long long n, unsigned per_million) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  unsigned h = (unsigned)i * 2654435761u;
  h ^= h >> 15;
  h *= 2246822519u;
  h ^= h >> 13;
  d2[i] = (h % 1000000u) < per_million ? 0u : 0xffffffffu;
}

// the early-exit grid's round: k_reach_round's body with the tile taken from the block index and no worklist
__global__ __launch_bounds__(256) void k_reach_round_grid(unsigned* g, ReachGeom q, unsigned* __restrict__ flags_cur, unsigned* __restrict__ flags_next,
                                                          unsigned long long* __restrict__ count_next, unsigned long long* __restrict__ relaxed) {
  __shared__ unsigned s_cells[REACH_HALO_CELLS];
  __shared__ unsigned s_moves[REACH_TILE_VOXELS];
  __shared__ unsigned s_seen[REACH_MOVES];
  const unsigned tid = threadIdx.x;
  const unsigned tile = blockIdx.x;
  if (flags_cur[tile] == 0u) return;  // (block-uniform: nobody writes this set during the round)
  __syncthreads();                    // (every thread has read the flag before thread 0 clears it)
  const unsigned tx = tile % q.ntx, ty = (tile / q.ntx) % q.nty, tz = tile / (q.ntx * q.nty);
  const unsigned ox = tx * REACH_TILE_X, oy = ty * REACH_TILE_Y, oz = tz * REACH_TILE_Z;
  if (tid == 0u) {
    flags_cur[tile] = 0u;
    atomicAdd(relaxed, 1ull);
  }
  if (tid < (unsigned)REACH_MOVES) s_seen[tid] = 0u;
  RelaxTile<unsigned> s{s_cells, s_moves};
  const ReachLoad ld{g};
  reach_tile_load<ReachValue>(s, ld, ox, oy, oz, q.X, q.Y, q.Z, tid, 256u);
  __syncthreads();
  reach_tile_moves<ReachValue>(s, tid, 256u);
  __syncthreads();
#pragma unroll 1
  for (unsigned sweep = 0u; sweep < (unsigned)REACH_TILE_VOXELS; ++sweep) {  // (bounded as in k_reach_round)
    const bool fell = reach_tile_sweep<ReachValue>(s, tid, 256u, q.cost, q.max_cost);
    if (!__syncthreads_or(fell ? 1 : 0)) break;
  }
  const unsigned seen_by = reach_tile_store<ReachValue>(s, ld, ReachStore{g}, ox, oy, oz, q.X, q.Y, q.Z, tid, 256u);
  if (seen_by) {
    for (int m = 0; m < REACH_MOVES; ++m)
      if ((seen_by >> m) & 1u) s_seen[m] = 1u;
  }
  __syncthreads();
  if (tid < (unsigned)REACH_MOVES && tid != (unsigned)REACH_CENTRE && s_seen[tid]) {
    const int nx = (int)tx + reach_dx((int)tid), ny = (int)ty + reach_dy((int)tid), nz = (int)tz + reach_dz((int)tid);
    if (nx >= 0 && nx < (int)q.ntx && ny >= 0 && ny < (int)q.nty && nz >= 0 && nz < (int)q.ntz)
      if (atomicAdd(&flags_next[((unsigned)nz * q.nty + (unsigned)ny) * q.ntx + (unsigned)nx], 1u) == 0u) atomicAdd(count_next, 1ull);
  }
}

int main(int argc, char** argv) {
  const unsigned N = argc > 1 ? (unsigned)atoi(argv[1]) : 512u, per_million = argc > 2 ? (unsigned)atoi(argv[2]) : 1000u;
  if (N < 8u || N > 1024u) return 2;
  const unsigned w[3] = {1u, 1u, 1u};
  ReachGeom q;
  reach_geom(N, N, N, w, 1u, REACH_MAX_COST, &q);
  const unsigned long long n = (unsigned long long)N * N * N, tiles = (unsigned long long)q.ntx * q.nty * q.ntz;
  unsigned* d2 = nullptr;
  void* scratch = nullptr;
  unsigned* d_seed = nullptr;
  CHECK(hipMalloc(&d2, n * 4));
  CHECK(hipMalloc(&scratch, reach_layout(q, nullptr, nullptr)));
  CHECK(hipMalloc(&d_seed, 4));
  ReachBufs b;
  reach_layout(q, scratch, &b);
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, 0, d2, n, per_million);
  const unsigned seed = (unsigned)(((unsigned long long)(N / 2) * N + N / 2) * N + N / 2);
  CHECK(hipMemset(d2 + seed, 0xff, 4));  // (the seed's voxel is passable)
  CHECK(hipMemcpy(d_seed, &seed, 4, hipMemcpyHostToDevice));
  CHECK(hipDeviceSynchronize());
  std::vector<unsigned> field[2] = {std::vector<unsigned>(n), std::vector<unsigned>(n)};
  for (int form = 0; form < 2; ++form) {
    double best = 1e30;
    unsigned long long rounds = 0, relaxed = 0;
    for (int rep = 0; rep < 4; ++rep) {  // (the first repetition loads the code; the best of the other three is printed)
      CHECK(launch_reach_init(0, d2, q, b));
      launch_reach_seed(0, q, b, d_seed, 1u);
      CHECK(hipMemset(b.counters + 6, 0, 8));
      CHECK(hipDeviceSynchronize());
      const auto t0 = std::chrono::steady_clock::now();
      unsigned long long n_active = 0;
      CHECK(hipMemcpy(&n_active, b.counters + 4, 8, hipMemcpyDeviceToHost));
      int cur = 0;
      rounds = relaxed = 0;
      while (n_active) {  // (ends: the field is a fixpoint after finitely many rounds; cut at REACH_MAX_ROUNDS)
        if (rounds >= REACH_MAX_ROUNDS) return 3;
        if (form == 0) {
          CHECK(launch_reach_round(0, q, b, cur, (unsigned)n_active));
          relaxed += n_active;
        } else {
          CHECK(hipMemsetAsync(b.counters + 4 + (cur ^ 1), 0, 8, 0));
          hipLaunchKernelGGL(k_reach_round_grid, dim3((unsigned)tiles), dim3(256), 0, 0, b.field, q, b.flags[cur], b.flags[cur ^ 1], b.counters + 4 + (cur ^ 1),
                             b.counters + 6);
          CHECK(hipGetLastError());
        }
        rounds += 1;
        cur ^= 1;
        CHECK(hipMemcpy(&n_active, b.counters + 4 + cur, 8, hipMemcpyDeviceToHost));
      }
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (rep > 0 && ms < best) best = ms;
      if (form == 1) CHECK(hipMemcpy(&relaxed, b.counters + 6, 8, hipMemcpyDeviceToHost));
    }
    CHECK(hipMemcpy(field[form].data(), b.field, n * 4, hipMemcpyDeviceToHost));
    printf("%s: %llu rounds, %llu tiles relaxed of %llu x rounds (%.2f %%), %.2f ms (best of 3)\n", form == 0 ? "compacted list " : "early-exit grid", rounds, relaxed,
           tiles, 100.0 * (double)relaxed / ((double)tiles * (double)(rounds ? rounds : 1)), best);
  }
  unsigned long long differ = 0, reached = 0;
  for (unsigned long long i = 0; i < n; ++i) {
    differ += field[0][i] != field[1][i] ? 1 : 0;
    reached += reach_is_value(field[0][i]) ? 1 : 0;
  }
  printf("%u^3, %u blocked per million: %llu voxels reached, %llu differ between the forms\n", N, per_million, reached, differ);
  (void)hipFree(d2);
  (void)hipFree(scratch);
  (void)hipFree(d_seed);
  return differ ? 1 : 0;
}
