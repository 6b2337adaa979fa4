// Grid-accelerated "K nearest within r": pn2_grid_build bins a batch of candidate clouds by cell once, pn2_grid_knn lets every query
// look at the 27 cells around its own.  The rule is in include/pn2.h under "grid kNN" and in numpy in tests/grid_knn_ref.py.
//
//   pn2_grid_build   six plain launches on the caller's stream, no thread ever waits for another thread's write:
//     grid_clear_kernel    every slot of every cloud's table (slot_table.h) to EMPTY with population 0; the cloud's header;
//     grid_count_kernel    one thread per candidate: the cell key (fp64, the rule of voxel_cell.h), pn2_slot_claim, 1 added to the
//                          slot's population; the row's slot is remembered (-1: the row is not in the grid);
//     grid_tile_kernel     one workgroup per tile of kTile slots: the tile's population;
//     grid_offsets_kernel  one wave per cloud: exclusive prefix sum over the tiles (pn2_wave_row_excl_scan), the cloud's indexed rows;
//     grid_start_kernel    one workgroup per tile: the exclusive prefix sum inside the tile (pn2_block_excl_scan) -> where each cell's
//                          records start (compact.h's pattern over populations instead of flags);
//     grid_fill_kernel     one thread per candidate: ONE 16-byte record (x, y, z, row index as bits) at the cell's cursor, which an
//                          atomicAdd advances: after the build a cell's records are [next - pop, next).  The rows that are not in the
//                          grid go behind the indexed ones, so that records [0, count) name every row of the cloud exactly once;
//                          the row's record position is remembered.
//   pn2_grid_knn     one launch, one query per lane: for each of the 27 neighbour cells in a fixed order a range check, a read-only
//                    probe (pn2_slot_find), a walk over the cell's records; the K best in registers (knn_select.h).
//   Which slot a key lands in and the order of the records inside a cell (and inside the tail) differ from run to run.  No output
//   does: populations and starts are integer sums, the selection compares (d2, index) PAIRS, so the K best are the same set in the
//   same order whatever order the candidates are met in, and `count` is an integer sum.  Every probe loop is bounded by the table's
//   capacity, every cell walk by the cell's population (clamped to the cloud's rows).  No float atomics.
//
// This file is built with -ffp-contract=off: the cell rule is two separately rounded fp64 operations, and the distance is
// pn2_chamfer_nn's difference form at D = 3 with its two fused steps spelled __builtin_fmaf.  The workspace's layout and the walk
// are in grid_walk.h, which icp.hip shares.
#include "grid_walk.h"
#include "wave_ops.h"

namespace {

__global__ __launch_bounds__(kThreads) void grid_clear_kernel(const int64_t *__restrict__ n_cand, int M, Work w) {
    const int b = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < (int64_t)w.cap; i += (int64_t)gridDim.x * kThreads)
        reinterpret_cast<uint4 *>(w.table + (int64_t)b * w.cap)[i] = pn2_slot_empty(0u, 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        Head h;
        h.count = pn2_rows_or_all(n_cand, b, M);
        h.indexed = h.tail = h.unused = 0;
        w.head[b] = h;
    }
}

__global__ __launch_bounds__(kThreads) void grid_count_kernel(const float *__restrict__ cand, int ldc, int M, const int64_t *__restrict__ n_cand,
                                                              Grid grid, Work w, int32_t *__restrict__ err) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= pn2_rows_or_all(n_cand, b, M)) return;
    const float *p = cand + ((int64_t)b * M + i) * ldc;
    unsigned long long key;
    int slot = -1;
    if (pn2_cell_key_of(p[0], p[1], p[2], grid, key)) {
        Slot *tab = w.table + (int64_t)b * w.cap;
        slot = pn2_slot_claim(tab, w.cap - 1u, key);                // (never -1: the table has twice as many slots as the cloud has rows)
        if (slot >= 0) atomicAdd(&tab[slot].pop, 1);
    } else if (err != nullptr) {
        atomicOr(err, PN2_GRID_ERR_CAND);
    }
    w.row_word[(int64_t)b * M + i] = slot;
}

// The populations of this thread's kPerThread consecutive slots of tile `tile` (0 beyond the table), their sum returned.
__device__ __forceinline__ int tile_pops(const Slot *__restrict__ tab, unsigned cap, int tile, int (&pop)[kPerThread]) {
    int sum = 0;
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
        const int64_t s = (int64_t)tile * kTile + (int64_t)threadIdx.x * kPerThread + r;
        pop[r] = s < (int64_t)cap ? tab[s].pop : 0;
        sum += pop[r];
    }
    return sum;
}

__global__ __launch_bounds__(kThreads) void grid_tile_kernel(Work w) {
    __shared__ int s_wave[kWaves];
    const int b = blockIdx.y, tile = blockIdx.x;
    int pop[kPerThread];
    const int mine = tile_pops(w.table + (int64_t)b * w.cap, w.cap, tile, pop);
    const int before = pn2_block_excl_scan(mine, s_wave);
    if (threadIdx.x == kThreads - 1) w.tile_sum[(int64_t)b * w.tiles + tile] = before + mine;
}

__global__ __launch_bounds__(PN2_WAVE) void grid_offsets_kernel(Work w) {
    const int b = blockIdx.x;
    const int total = pn2_wave_row_excl_scan(w.tile_sum + (int64_t)b * w.tiles, w.tile_start + (int64_t)b * w.tiles, w.tiles);   // at most M < 2^31
    if (threadIdx.x == 0) w.head[b].indexed = total;
}

__global__ __launch_bounds__(kThreads) void grid_start_kernel(Work w) {
    __shared__ int s_wave[kWaves];
    const int b = blockIdx.y, tile = blockIdx.x;
    Slot *tab = w.table + (int64_t)b * w.cap;
    int pop[kPerThread];
    const int mine = tile_pops(tab, w.cap, tile, pop);
    int at = w.tile_start[(int64_t)b * w.tiles + tile] + pn2_block_excl_scan(mine, s_wave);
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
        const int64_t s = (int64_t)tile * kTile + (int64_t)threadIdx.x * kPerThread + r;
        if (s < (int64_t)w.cap) tab[s].next = at;
        at += pop[r];
    }
}

__global__ __launch_bounds__(kThreads) void grid_fill_kernel(const float *__restrict__ cand, int ldc, int M, Work w) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    Head *head = w.head + b;
    if (i >= head->count) return;                                   // (the count the first launch read: <= M)
    const int slot = w.row_word[(int64_t)b * M + i];
    const int at = slot >= 0 ? atomicAdd(&w.table[(int64_t)b * w.cap + slot].next, 1) : head->indexed + atomicAdd(&head->tail, 1);
    const float *p = cand + ((int64_t)b * M + i) * ldc;
    if (at >= 0 && at < M) w.rec[(int64_t)b * M + at] = make_float4(p[0], p[1], p[2], __int_as_float((int)i));       // (always: the populations add up to the indexed rows)
    w.row_word[(int64_t)b * M + i] = at;
}

// One query per lane.  A self-search (query == nullptr) takes its point from the records: lane i serves row i, or, `sorted`, the
// i-th RECORD and writes at that record's row -- neighbouring lanes then share cells.  Everything read from the workspace that is
// used as an address is checked against M first: a workspace that no build filled cannot send a lane out of bounds.
template <int CAP>
__global__ __launch_bounds__(kThreads) void grid_knn_kernel(const float *__restrict__ query, int ldq, int N, int M, int K, float max_d2,
                                                            const int64_t *__restrict__ n_query, Grid grid, Work w, int sorted,
                                                            int64_t *__restrict__ idx, float *__restrict__ dist,
                                                            int32_t *__restrict__ count, int32_t *__restrict__ err) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const float4 *__restrict__ rec = w.rec + (int64_t)b * M;
    float qx, qy, qz;
    int64_t row = i;
    if (query == nullptr) {
        const int n = w.head[b].count;
        if (i >= n || i >= M) return;
        int at = (int)i;
        if (!sorted) at = w.row_word[(int64_t)b * M + i];
        if (at < 0 || at >= M) return;
        const float4 r = rec[at];
        qx = r.x; qy = r.y; qz = r.z;
        if (sorted) row = __float_as_int(r.w);
        if (row < 0 || row >= M) return;
    } else {
        if (i >= pn2_rows_or_all(n_query, b, N)) return;
        const float *q = query + ((int64_t)b * N + i) * ldq;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    float bd[CAP];
    int bi[CAP];
#pragma unroll
    for (int s = 0; s < CAP; ++s) { bd[s] = INFINITY; bi[s] = M; }
    int took = 0;
    if (!pn2_grid_walk<CAP>(qx, qy, qz, grid, w, b, M, max_d2, bd, bi, took) && err != nullptr) atomicOr(err, PN2_GRID_ERR_QUERY);
    const size_t o = ((size_t)b * N + (size_t)row) * K;
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        if (s < K) {
            idx[o + s] = bi[s];
            if (dist != nullptr) dist[o + s] = bd[s];
        }
    }
    if (count != nullptr) count[(size_t)b * N + (size_t)row] = took;
}

template <int CAP>
int launch_grid_knn(const float *query, int ldq, int B, int N, int M, int K, float max_d2, const int64_t *n_query, const Grid &grid,
                    const Work &w, int sorted, int64_t *idx, float *dist, int32_t *count, int32_t *err, hipStream_t s) {
    hipLaunchKernelGGL(grid_knn_kernel<CAP>, dim3((unsigned)pn2_cdiv(N, kThreads), (unsigned)B), dim3(kThreads), 0, s, query, ldq, N, M, K,
                       max_d2, n_query, grid, w, sorted, idx, dist, count, err);
    return pn2_launch_status();
}

}  // namespace

extern "C" {

int64_t pn2_grid_workspace_bytes(int B, int64_t M) {
    int64_t bytes = PN2_EINVAL;
    if (grid_shape_ok(B, M)) grid_work(B, M, nullptr, &bytes);
    return bytes;
}

int pn2_grid_build(const float *cand, int ldc, int B, int M, const int64_t *n_cand, const double *origin, const double *cell, int32_t *err,
                   void *workspace, pn2_stream_t stream) {
    PN2_CHECK_ARG(cand && origin && cell && workspace);
    PN2_CHECK_ARG(grid_shape_ok(B, M) && ldc >= 3 && ldc <= 16);
    PN2_CHECK_ARG(pn2_aligned(cand, 4) && pn2_aligned(workspace, 16));
    Grid grid;
    PN2_CHECK_ARG(pn2_grid_from(origin, cell, grid));
    const Work w = grid_work(B, M, workspace);
    const hipStream_t s = pn2_s(stream);
    const dim3 by_row((unsigned)pn2_cdiv(M, kThreads), (unsigned)B), by_tile((unsigned)w.tiles, (unsigned)B);
    hipLaunchKernelGGL(grid_clear_kernel, dim3(pn2_slot_clear_blocks(w.cap), (unsigned)B), dim3(kThreads), 0, s, n_cand, M, w);
    hipLaunchKernelGGL(grid_count_kernel, by_row, dim3(kThreads), 0, s, cand, ldc, M, n_cand, grid, w, err);
    hipLaunchKernelGGL(grid_tile_kernel, by_tile, dim3(kThreads), 0, s, w);
    hipLaunchKernelGGL(grid_offsets_kernel, dim3((unsigned)B), dim3(PN2_WAVE), 0, s, w);
    hipLaunchKernelGGL(grid_start_kernel, by_tile, dim3(kThreads), 0, s, w);
    hipLaunchKernelGGL(grid_fill_kernel, by_row, dim3(kThreads), 0, s, cand, ldc, M, w);
    return pn2_launch_status();
}

int pn2_grid_knn(const float *query, int ldq, int B, int N, int M, int K, float max_d2, const int64_t *n_query, const double *origin,
                 const double *cell, const void *workspace, int flags, int64_t *idx, float *dist, int32_t *count, int32_t *err,
                 pn2_stream_t stream) {
    PN2_CHECK_ARG(origin && cell && workspace && idx);
    PN2_CHECK_ARG(grid_shape_ok(B, M) && N > 0 && N <= 0x7FFFFF00 && K >= 1);
    PN2_CHECK_ARG(query != nullptr ? (ldq >= 3 && ldq <= 16) : N == M);
    PN2_CHECK_ARG((flags & ~PN2_GRID_VISIT_SORTED) == 0);
    PN2_CHECK_ARG(pn2_aligned(query, 4) && pn2_aligned(workspace, 16));
    Grid grid;
    PN2_CHECK_ARG(pn2_grid_from(origin, cell, grid));
    if (K > 32) return PN2_EUNSUPPORTED;
    const Work w = grid_work(B, M, const_cast<void *>(workspace));      // (the query kernel only reads it)
    const int sorted = query == nullptr && (flags & PN2_GRID_VISIT_SORTED) != 0;
    const hipStream_t s = pn2_s(stream);
    if (K <= 4) return launch_grid_knn<4>(query, ldq, B, N, M, K, max_d2, n_query, grid, w, sorted, idx, dist, count, err, s);
    if (K <= 8) return launch_grid_knn<8>(query, ldq, B, N, M, K, max_d2, n_query, grid, w, sorted, idx, dist, count, err, s);
    if (K <= 16) return launch_grid_knn<16>(query, ldq, B, N, M, K, max_d2, n_query, grid, w, sorted, idx, dist, count, err, s);
    return launch_grid_knn<32>(query, ldq, B, N, M, K, max_d2, n_query, grid, w, sorted, idx, dist, count, err, s);
}

}  // extern "C"
