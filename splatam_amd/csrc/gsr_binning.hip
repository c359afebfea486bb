// gsr_binning.hip -- from preprocess's tile counts to the tile buckets the render sorts (the reference's
// InclusiveSum, duplicateWithKeys and identifyTileRanges, rasterizer_impl.cu:277, 70-111, 116-138, without a
// global sort).  In launch order:
//   tile_colscan_kernel      column scan of the [workgroup x tile] count matrix: each workgroup's offset in
//                            each tile's bucket, and the tile totals
//   duplicate_bucket_kernel  every workgroup scans the workgroup sums and tile totals in its prologue
//                            (workgroup 0 publishes ranges, counters, status and the render schedule,
//                            tile_plan), then places its Gaussians' instances in their tiles' buckets
// The scan of the totals as a stage of its own (scan_counts_body) runs where the duplicate does not do it: as
// the colscan's TAIL when GSR_FORCE_RADIX skips the bucketed duplicate (gsr_radix.hip), and as
// scan_counts_kernel on the global-atomic counts of a frame with more than MAX_LDS_TILES tiles.
#include "gsr_clock.h"
#include "gsr_dispatch.h"
#include "gsr_launch.h"
#include "gsr_layout.h"
#include "gsr_wave.h"

namespace gsr {

constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_ITEMS = 4;

// One workgroup: exclusive scan of the per-workgroup tile sums (instance
// offsets, total = num_rendered) and of the per-tile instance counts, which
// directly gives every tile's [start, end) in the tile-major sorted list
// (identifyTileRanges, rasterizer_impl.cu:116-138, without reading keys).
// AGENT_TILES: the tile counts were published by other workgroups of the same
// launch (tile_colscan_kernel's last workgroup) and are read with agent-scope loads.
template <bool AGENT_TILES>
__device__ void scan_counts_body(const uint32_t* __restrict__ wgsum, uint32_t* __restrict__ blocksums, uint32_t nb,
                                 const uint32_t* __restrict__ tile_count, uint32_t tile_stride, uint32_t ntiles,
                                 uint2* __restrict__ ranges, uint32_t* __restrict__ counters, uint32_t sort_cap,
                                 uint32_t* __restrict__ status) {
    // Writes all four counters (no reset needed): [0] num_rendered, [1] prefiltered violation
    // (top bits of the workgroup sums), [2] longest tile list, [3] sort_cap; and a copy to
    // `status` (static mode).
    __shared__ uint32_t wsums[SCAN_THREADS / 64];
    __shared__ uint32_t s_carry, s_max, s_viol;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_viol = 0;
    for (int pass = 0; pass < 2; pass++) {
        const uint32_t n = pass == 0 ? nb : ntiles;
        const uint32_t* src = pass == 0 ? wgsum : tile_count;
        if (tid == 0) { s_carry = 0; s_max = 0; }
        __syncthreads();
        uint32_t vmax = 0, viol = 0;
        for (uint32_t base = 0; base < n; base += SCAN_THREADS * SCAN_ITEMS) {
            uint32_t x[SCAN_ITEMS], sum = 0;
            const uint32_t i0 = base + (uint32_t)tid * SCAN_ITEMS;
#pragma unroll
            for (int k = 0; k < SCAN_ITEMS; k++) {
                const uint32_t* ps = src + (size_t)(i0 + k) * (pass == 0 ? 1u : tile_stride);
                x[k] = (i0 + k < n) ? ((AGENT_TILES && pass == 1) ? ld_agent(ps) : *ps) : 0u;
                if (pass == 0) {  // workgroup sums carry the prefiltered-violation flag in bit 31
                    viol |= x[k] >> 31;
                    x[k] &= 0x7fffffffu;
                }
                sum += x[k];
                vmax = max(vmax, x[k]);
            }
            uint32_t incl = wave_incl_scan(sum);
            if (lane == 63) wsums[w] = incl;
            __syncthreads();
            if (w == 0) {
                uint32_t ws = (lane < SCAN_THREADS / 64) ? wsums[lane] : 0u;
                uint32_t wi = wave_incl_scan(ws);
                if (lane < SCAN_THREADS / 64) wsums[lane] = wi - ws;
            }
            __syncthreads();
            uint32_t run = s_carry + wsums[w] + incl - sum;
#pragma unroll
            for (int k = 0; k < SCAN_ITEMS; k++) {
                if (i0 + k < n) {
                    if (pass == 0) blocksums[i0 + k] = run;
                    else ranges[i0 + k] = make_uint2(run, run + x[k]);
                }
                run += x[k];
            }
            __syncthreads();
            if (tid == SCAN_THREADS - 1) s_carry = run;
            __syncthreads();
        }
        atomicMax(&s_max, vmax);
        if (viol) atomicOr(&s_viol, 1u);
        __syncthreads();
        if (tid == 0) {
            if (pass == 0) {
                counters[0] = s_carry;
                counters[1] = s_viol;
                if (status) status_merge(status, s_carry, s_viol, 0u, 0u);
            } else {
                counters[2] = s_max;
                counters[3] = sort_cap;  // longest list the tile sort will handle (BwdGuard)
                if (status) status_merge(status, 0u, 0u, s_max, sort_cap);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(SCAN_THREADS)
scan_counts_kernel(const uint32_t* __restrict__ wgsum, uint32_t* __restrict__ blocksums, uint32_t nb,
                   const uint32_t* __restrict__ tile_count,
                   uint32_t tile_stride, uint32_t ntiles, uint2* __restrict__ ranges,
                   uint32_t* __restrict__ counters, uint32_t sort_cap, uint32_t* __restrict__ status) {
    scan_counts_body<false>(wgsum, blocksums, nb, tile_count, tile_stride, ntiles, ranges, counters, sort_cap, status);
}

hipError_t launch_scan_counts(GeomPtrs geo, int nb, const uint32_t* tile_count, int tile_stride, int ntiles,
                              uint2* ranges, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, geo.wgsum, geo.blocksums, (uint32_t)nb,
                       tile_count,
                       (uint32_t)tile_stride, (uint32_t)ntiles, ranges, geo.counters, (uint32_t)TILE_SORT_CAP,
                       status);
    return hipGetLastError();
}

// ------------------------------------------------------------ column scan --
// Column scan of the [workgroup x tile] count matrix: in place, every entry
// becomes the workgroup's offset inside its tile's bucket; tot[t] = tile total.
// One workgroup per 16 tiles, 64 row segments each (coalesced across tiles): a
// frame's 1200 tiles give 75 workgroups, and a thread's <= CS_RQ column entries
// are loaded once, all in flight, and kept in registers for the offset pass
// (the previous 64-tile x 16-segment shape ran 19 workgroups of two dependent
// load passes: 16.5 us at config 3).
// Two shapes: 16 tiles x 64 parts (64-B row segments) for count matrices of <= 512 rows, 32 x 32
// (128-B segments, <= 32 rows per thread) above: 5.2 vs 5.8 us at config 3 (293 rows), 19.1 vs
// 16.2 us at config 4 (977 rows).
#ifndef GSR_CS_ROWS_SMALL
#define GSR_CS_ROWS_SMALL 640  // (config 3 has 586 rows of 512 Gaussians)
#endif
constexpr int CS_THREADS = 1024, CS_ROWS_SMALL = GSR_CS_ROWS_SMALL;
template <int CT>
struct ColscanShape {
    static constexpr int TILES = CT, PARTS = CS_THREADS / CT, RQ = PARTS == 64 ? 16 : 32;
};

// TAIL: ... and, in the same launch, the scan of scan_counts_kernel: the
// workgroups publish their tile totals (agent-scope stores), the last one to
// finish scans the workgroup sums and the tile totals (the arrival counter is
// GeomLayout counters[4], zeroed by preprocess).  Without TAIL (the bucketed
// path) every duplicate_bucket workgroup does those scans itself in its
// prologue, which removes this launch's serial tail (arrival + one-workgroup
// scan: ~10 us of latency at config 3).
template <bool TAIL, int CT>
__device__ __forceinline__ void tile_colscan_body(uint32_t* __restrict__ counts, int nb, int ntiles,
                                                  uint32_t* __restrict__ tot, GeomPtrs geo, uint2* __restrict__ ranges,
                                                  uint32_t sort_cap, uint32_t* __restrict__ status) {
    constexpr int CS_TILES = ColscanShape<CT>::TILES, CS_PARTS = ColscanShape<CT>::PARTS, CS_RQ = ColscanShape<CT>::RQ;
    __shared__ uint32_t s_part[CS_PARTS][CS_TILES];
    const int tl = threadIdx.x % CS_TILES, q = threadIdx.x / CS_TILES;
    const int t = blockIdx.x * CS_TILES + tl;
    const int rq = (nb + CS_PARTS - 1) / CS_PARTS;
    const int b0 = min(nb, q * rq), b1 = min(nb, b0 + rq);
    uint32_t sum = 0;
    uint32_t vals[CS_RQ];
    const bool in_regs = rq <= CS_RQ;
    if (t < ntiles) {
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < CS_RQ; k++) {
                vals[k] = b0 + k < b1 ? counts[(size_t)(b0 + k) * ntiles + t] : 0u;
                sum += vals[k];
            }
        } else {
#pragma unroll 4
            for (int b = b0; b < b1; b++) sum += counts[(size_t)b * ntiles + t];
        }
    }
    s_part[q][tl] = sum;
    __syncthreads();
    {  // each wave scans 64 / CS_PARTS tile columns' part sums (lane = part) in place: exclusive prefixes
        static_assert(CS_PARTS == 64 || CS_PARTS == 32, "one or two tile columns per wave");
        constexpr int CPW = 64 / CS_PARTS;  // columns per wave
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int part = lane % CS_PARTS, colw = CPW * w + lane / CS_PARTS;
        const uint32_t v = s_part[part][colw];
        uint32_t inc = wave_incl_scan(v);
        if (CPW == 2) {  // the upper half-wave's column starts after the lower column's total
            const uint32_t lo_tot = (uint32_t)__shfl((int)inc, 31);
            if (lane >= 32) inc -= lo_tot;
        }
        s_part[part][colw] = inc - v;
    }
    __syncthreads();
    uint32_t run = s_part[q][tl];
    if (t < ntiles) {
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < CS_RQ; k++)
                if (b0 + k < b1) {
                    counts[(size_t)(b0 + k) * ntiles + t] = run;
                    run += vals[k];
                }
        } else {
#pragma unroll 4
            for (int b = b0; b < b1; b++) {
                const uint32_t v = counts[(size_t)b * ntiles + t];
                counts[(size_t)b * ntiles + t] = run;
                run += v;
            }
        }
        if (q == CS_PARTS - 1) {
            if (TAIL) st_agent(&tot[t], run);
            else tot[t] = run;
        }
    }
    if (!TAIL) return;
    if (!last_block_arrive(&geo.counters[4])) return;
    scan_counts_body<true>(geo.wgsum, geo.blocksums, (uint32_t)nb, tot, 1u, (uint32_t)ntiles, ranges, geo.counters,
                           sort_cap, status);
}
template <bool TAIL, int CT, bool CLK>
__global__ void __launch_bounds__(CS_THREADS)
tile_colscan_kernel(uint32_t* __restrict__ counts, int nb, int ntiles, uint32_t* __restrict__ tot, GeomPtrs geo,
                    uint2* __restrict__ ranges, uint32_t sort_cap, uint32_t* __restrict__ status,
                    unsigned long long* clk, Gate gate) {
    if (gate.off()) return;
    if constexpr (CLK) kclock_begin(clk);
    tile_colscan_body<TAIL, CT>(counts, nb, ntiles, tot, geo, ranges, sort_cap, status);
    if constexpr (CLK) kclock_end(clk);
}

struct PickTileColscan {
    template <bool TAIL, bool WIDE, bool CLK>
    auto operator()() const { return &tile_colscan_kernel<TAIL, WIDE ? 32 : 16, CLK>; }
};

hipError_t launch_tile_colscan(uint32_t* counts, int nb, int ntiles, uint32_t* tot, GeomPtrs geo, uint2* ranges,
                               uint32_t* status, bool tail, hipStream_t s, unsigned long long* clk, Gate gate) {
    static_assert(CS_THREADS == SCAN_THREADS, "the last colscan workgroup runs the scan body");
    const bool wide = nb > CS_ROWS_SMALL;
    const int ct = wide ? 32 : 16;
    const auto k = dispatch_bools(PickTileColscan{}, tail, wide, clk != nullptr);
    hipLaunchKernelGGL(k, dim3((ntiles + ct - 1) / ct), dim3(CS_THREADS), 0, s, counts, nb, ntiles, tot, geo, ranges,
                       (uint32_t)TILE_SORT_CAP, status, clk, gate);
    return hipGetLastError();
}

// ---- render schedule ---------------------------------------------------------
// All of a frame's render workgroups are resident at once (e.g. 1200 tiles on 256
// CUs at 5 workgroups per CU), workgroup i is dispatched to XCD i mod 8 and, inside
// it, round-robin over the XCD's CUs: workgroups i and i + ncu share a CU.  A render
// kernel therefore lasts as long as its most loaded CU (measured: the per-CU sum of
// tile work spread 0.81-1.18x of the mean with the row-major order, kernel span set
// by the top; tools/wgtime.py).  tile_plan deals the tiles, in descending order of
// list length (the render cost: 0.998 correlation with the tile's contributing
// pairs), to workgroup slots in rounds, alternating direction, so every CU's tiles
// add up to about the same work.  With n = q * ncu + m tiles, m CUs render q + 1
// tiles and ncu - m render q (config 3: 176 CUs x 5, 80 x 4; the per-CU end times
// follow the tile count first, `profiles/r4s_wgtime_fused.json`): the CUs with q
// tiles take the q (ncu - m) longest lists, dealt over their own q rounds, and the
// others the rest over q + 1 rounds.  Counting sort over length buckets of 4: ties
// land in arbitrary order, which changes only which workgroup renders a tile, never
// its results.
constexpr int PLAN_BUCKETS = 1024, PLAN_SHIFT = 2;
__device__ __forceinline__ uint32_t plan_bucket(uint32_t len) {  // descending length -> ascending bucket
    return (uint32_t)(PLAN_BUCKETS - 1) - min(len >> PLAN_SHIFT, (uint32_t)(PLAN_BUCKETS - 1));
}
__device__ __forceinline__ uint32_t plan_slot(uint32_t p, uint32_t n, uint32_t ncu) {
    const uint32_t q = n / ncu, m = n - q * ncu, heavy = q * (ncu - m);
    // group: CUs [g0, g0 + gs) (slot s renders on CU class s mod ncu), pp = position inside the group
    const bool hv = p < heavy;
    const uint32_t g0 = hv ? m : 0u, gs = hv ? ncu - m : m, pp = hv ? p : p - heavy;
    const uint32_t rd = pp / gs, k = pp - rd * gs;
    return rd * ncu + g0 + ((rd & 1u) ? gs - 1u - k : k);
}
// one workgroup of NT threads (PLAN_BUCKETS / NT consecutive buckets per thread); s_hist:
// PLAN_BUCKETS words of LDS, s_wsum: NT / 64
// TPT > 0: the tile totals come from registers, tv[k] = total of tile t0 + k (t0 + k < t1) -- no
// reload of `tot` after the caller's stores (a load issued after a store waits for it too)
template <int NT, int TPT = 0>
__device__ void tile_plan(const uint32_t* __restrict__ tot, int ntiles, int ncu, uint32_t* __restrict__ order,
                          uint32_t* s_hist, uint32_t* s_wsum, const uint32_t* tv = nullptr, int t0 = 0,
                          int t1 = 0) {
    constexpr int BPT = PLAN_BUCKETS / NT;
    static_assert(BPT * NT == PLAN_BUCKETS, "buckets per thread");
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int k = 0; k < BPT; k++) s_hist[tid * BPT + k] = 0u;
    __syncthreads();
    if constexpr (TPT > 0) {
#pragma unroll
        for (int k = 0; k < TPT; k++)
            if (t0 + k < t1) atomicAdd(&s_hist[plan_bucket(tv[k])], 1u);
    } else {
        for (int u = tid; u < ntiles; u += NT) atomicAdd(&s_hist[plan_bucket(tot[u])], 1u);
    }
    __syncthreads();
    uint32_t c[BPT], cs = 0;
#pragma unroll
    for (int k = 0; k < BPT; k++) {
        c[k] = s_hist[tid * BPT + k];
        cs += c[k];
    }
    const uint32_t incl = wave_incl_scan(cs);
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    uint32_t run = incl - cs;
    for (int k = 0; k < w; k++) run += s_wsum[k];
#pragma unroll
    for (int k = 0; k < BPT; k++) {  // exclusive: first position of each bucket
        s_hist[tid * BPT + k] = run;
        run += c[k];
    }
    __syncthreads();
    if constexpr (TPT > 0) {
#pragma unroll
        for (int k = 0; k < TPT; k++)
            if (t0 + k < t1) {
                const uint32_t p = atomicAdd(&s_hist[plan_bucket(tv[k])], 1u);
                order[plan_slot(p, (uint32_t)ntiles, (uint32_t)ncu)] = (uint32_t)(t0 + k);
            }
    } else {
        for (int u = tid; u < ntiles; u += NT) {
            const uint32_t p = atomicAdd(&s_hist[plan_bucket(tot[u])], 1u);
            order[plan_slot(p, (uint32_t)ntiles, (uint32_t)ncu)] = (uint32_t)u;
        }
    }
}

__global__ void identity_order_kernel(uint32_t* __restrict__ order, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) order[i] = (uint32_t)i;
}
hipError_t launch_identity_order(uint32_t* order, int ntiles, hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(identity_order_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, s, order, ntiles);
    return hipGetLastError();
}

// ------------------------------------------------------ bucketed duplicate --
// DUP_T lanes per workgroup, each placing the instances of DUP_G consecutive Gaussians of a count-matrix
// row (DUP_G = 2 for rows of 1024, 1 for rows of 512): at 1024 lanes (98 VGPRs, one workgroup per CU) a
// frame's ~300 workgroups took two dispatch rounds on 37 CUs; at 512 two workgroups share a CU (one
// round).  Forcing 1024-lane workgroups to 64 VGPRs instead spilled and was slower.
constexpr int DUP_T = 512;
#ifndef GSR_DUP_LOOP_MAX
#define GSR_DUP_LOOP_MAX 16  // rows whose Gaussians touch at most this many tiles place instances per lane
#endif
// the snapshot the host reads after the duplicate (Camera::host_snap): two 16-B vector stores to the coherent
// pinned buffer, made visible to the host by the kernel's end-of-kernel release
__device__ __forceinline__ void store_host_snap(uint32_t* snap, uint4 lo, uint4 hi) {
    reinterpret_cast<uint4*>(snap)[0] = lo;
    reinterpret_cast<uint4*>(snap)[1] = hi;
}
// gated geometry reuse, equal geometry: the duplicate is skipped, and its workgroup 0 hands the counters the reuse
// copy wrote (the previous call's [0..3], this call's [4..7]) to the host instead
__device__ __forceinline__ void dup_gate_off_snap(const Camera& cam, const GeomPtrs& geo) {
    if (cam.host_snap && blockIdx.x == 0 && threadIdx.x == 0)
        store_host_snap(cam.host_snap, *reinterpret_cast<const uint4*>(geo.counters),
                        *reinterpret_cast<const uint4*>(geo.counters + 4));
}
// Bucketed duplicate: every instance goes straight into its tile's bucket
// (slot from a per-tile cursor), keyed (depth bits << 32 | Gaussian id).  The
// order inside a bucket is arbitrary; render_fwd (tile_sort_bucket) restores the reference
// order (depth, then id: cub's stable LSD sort, rasterizer_impl.cu:304-309).
template <bool LDS_HIST, int DUP_G, bool EXACT>
__device__ __forceinline__ void duplicate_bucket_body(Camera cam, int P, GeomPtrs geo, uint2* __restrict__ ranges,
                                                      const uint32_t* __restrict__ tot, uint32_t* __restrict__ cursor,
                                                      int ntiles, uint64_t* __restrict__ keys,
                                                      uint64_t* __restrict__ point_list, SpecGuard guard,
                                                      uint32_t sort_cap, uint32_t* __restrict__ status,
                                                      uint32_t* __restrict__ s_cur) {
    // LDS_HIST: cursor = the column-scanned count matrix; this workgroup's
    // instances of tile t go to start[t] + cursor[block][t] + (LDS rank)
    // Culled instances (Camera::cull) are in no bucket, so the tile lists fill point_list[0, L) with L <
    // num_rendered; the tail [L, num_rendered) is written too, so every one of the num_rendered entries the
    // forward returns is a valid Gaussian id with an empty block mask (PointEntry = mask << 32 | id):
    //   EXACT (the dynamic, drop-in forward): the culled instances themselves, in (Gaussian, rect tile) order --
    //     the ids are then the reference's multiset (Gaussian i listed tiles_touched(i) times);
    //   else (static mode: the library is the only reader): padding -- slot u of the tail holds the Gaussian
    //     owning rect instance slot u (offsets[i] <= u < offsets[i] + tiles[i]), which needs no global prefix of
    //     the culled counts (that bookkeeping cost the kernel 16 VGPRs and a second dispatch round).
    constexpr int ROW = DUP_G * DUP_T;  // Gaussians per count-matrix row (1 << cam.pre_shift)
    __shared__ uint32_t s_incl[ROW];
    __shared__ uint32_t s_x0[ROW], s_y0[ROW], s_w[ROW], s_depth[ROW], s_live[ROW];
    __shared__ uint32_t s_cx[EXACT ? ROW : 1];
    __shared__ uint32_t wsum[DUP_T / 64], s_tmax[DUP_T / 64], s_cws[DUP_T / 64];
    __shared__ uint32_t s_cred[2][DUP_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i0 = blockIdx.x * ROW + DUP_G * tid;  // this lane's Gaussians i0 .. i0 + DUP_G - 1
    // the Gaussians' tile counts and rects, loaded ahead of the prologue's loads (one round trip)
    uint32_t t[DUP_G];
    uint4 r[DUP_G];
#pragma unroll
    for (int g = 0; g < DUP_G; g++) {
        t[g] = (i0 + g < P) ? geo.tiles[i0 + g] : 0u;
        r[g] = (i0 + g < P) ? geo.bin[i0 + g] : make_uint4(0u, 0u, 0u, 0u);  // (rect lo, rect hi, depth bits, tiles)
    }
    uint32_t base, ctail = 0, ltot = 0xFFFFFFFFu;  // ltot: L, the lists' total (padding tail)
    if (LDS_HIST) {
        // The scans of scan_counts_body, redone by every workgroup (the inputs are
        // a few KB, L2-resident): this workgroup's instance base from the raw
        // workgroup totals, num_rendered, the prefiltered flag, and the exclusive
        // scan of the tile totals (bucket starts).  Workgroup 0 publishes them
        // (ranges, counters, status) for the later launches and the host.
        constexpr int TPT = 4;  // tiles per thread kept in registers (<= 4 DUP_T tiles), else staged in LDS
        __shared__ uint32_t s_red[5][DUP_T / 64];
        const uint32_t b = blockIdx.x, nb = gridDim.x;
        const int per = (ntiles + DUP_T - 1) / DUP_T;  // contiguous tiles per thread
        const int t0 = min(ntiles, tid * per), t1 = min(ntiles, t0 + per);
        const bool in_regs = per <= TPT;
        uint32_t tv[TPT], cv[TPT];
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            const bool ok = in_regs && t0 + k < t1;
            tv[k] = ok ? tot[t0 + k] : 0u;
            cv[k] = ok ? cursor[(size_t)b * ntiles + t0 + k] : 0u;
        }
        uint32_t pre = 0, all = 0, viol = 0, vmax = 0, cpre = 0, call = 0;
        // two workgroup sums per trip, both loads issued before either is used (config 3: 586 rows, so some
        // lanes read two -- one memory round trip instead of two ahead of the workgroup's first barrier)
        for (uint32_t k = tid; k < nb; k += 2 * DUP_T) {
            const uint32_t k2 = k + DUP_T;
            const uint32_t v = geo.wgsum[k], v2 = k2 < nb ? geo.wgsum[k2] : 0u;
            // (EXACT: preprocess wrote wgcull; loaded unconditionally, with the workgroup sums)
            const uint32_t c = EXACT ? geo.wgcull[k] : 0u, c2 = (EXACT && k2 < nb) ? geo.wgcull[k2] : 0u;
            viol |= (v | v2) >> 31;
            all += (v & 0x7fffffffu) + (v2 & 0x7fffffffu);
            pre += (k < b ? (v & 0x7fffffffu) : 0u) + (k2 < b ? (v2 & 0x7fffffffu) : 0u);
            if (EXACT) {
                call += c + c2;
                cpre += (k < b ? c : 0u) + (k2 < b ? c2 : 0u);
            }
        }
        uint32_t csum = 0;
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < TPT; k++) {
                csum += tv[k];
                vmax = max(vmax, tv[k]);
            }
        } else {
            for (int u = t0; u < t1; u++) {
                const uint32_t v = tot[u];
                s_cur[u] = v;
                csum += v;
                vmax = max(vmax, v);
            }
        }
        const uint32_t cincl = wave_incl_scan(csum);
        pre = wave_sum_u32(pre);
        all = wave_sum_u32(all);
        viol = wave_max_u32(viol);
        vmax = wave_max_u32(vmax);
        if (EXACT && cam.cull) {
            cpre = wave_sum_u32(cpre);
            call = wave_sum_u32(call);
        }
        if (lane == 0) {
            s_red[0][w] = pre;
            s_red[1][w] = all;
            s_red[2][w] = viol;
            s_red[3][w] = vmax;
            if (EXACT) {
                s_cred[0][w] = cpre;
                s_cred[1][w] = call;
            }
        }
        if (lane == 63) s_red[4][w] = cincl;
        __syncthreads();
        uint32_t woff = 0, lsum = 0;
        pre = all = viol = vmax = cpre = call = 0;
#pragma unroll
        for (int k = 0; k < DUP_T / 64; k++) {
            pre += s_red[0][k];
            all += s_red[1][k];
            viol |= s_red[2][k];
            vmax = max(vmax, s_red[3][k]);
            woff += k < w ? s_red[4][k] : 0u;
            if (!EXACT) lsum += s_red[4][k];
            if (EXACT) {
                cpre += s_cred[0][k];
                call += s_cred[1][k];
            }
        }
        if (EXACT) ctail = all - call + cpre;  // this workgroup's first culled instance in point_list
        if (!EXACT) ltot = lsum;
        uint32_t run = woff + cincl - csum;  // bucket start of this thread's first tile
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < TPT; k++)
                if (t0 + k < t1) {
                    if (b == 0) ranges[t0 + k] = make_uint2(run, run + tv[k]);
                    s_cur[t0 + k] = run + cv[k];
                    run += tv[k];
                }
        } else {
            for (int u = t0; u < t1; u++) {
                const uint32_t v = s_cur[u];
                if (b == 0) ranges[u] = make_uint2(run, run + v);
                s_cur[u] = run + cursor[(size_t)b * ntiles + u];
                run += v;
            }
        }
        if (tid == 0) {
            geo.blocksums[b] = pre;
            if (b == 0) {
                // [0] num_rendered [1] prefiltered violation [2] longest tile list [3] sort cap
                geo.counters[0] = all;
                geo.counters[1] = viol;
                geo.counters[2] = vmax;
                geo.counters[3] = sort_cap;
                if (status) status_merge(status, all, viol, vmax, sort_cap);
                if (cam.host_snap)  // (Camera::host_snap; [4..7] were final before this launch)
                    store_host_snap(cam.host_snap, make_uint4(all, viol, vmax, sort_cap),
                                    *reinterpret_cast<const uint4*>(geo.counters + 4));
            }
        }
        if (b == 0 && cam.tile_order_out) {
            __shared__ uint32_t s_plan[PLAN_BUCKETS];
            if (in_regs)
                tile_plan<DUP_T, TPT>(tot, ntiles, cam.sched_cus, cam.tile_order_out, s_plan, wsum, tv, t0, t1);
            else
                tile_plan<DUP_T>(tot, ntiles, cam.sched_cus, cam.tile_order_out, s_plan, wsum);
        }
        base = pre;
        if (all > guard.cap_inst || vmax > guard.cap_tile) return;  // workgroup-uniform
    } else {
        if (guard.overflow()) return;
        base = geo.blocksums[blockIdx.x];
        if (!EXACT && ntiles > 0) ltot = ranges[ntiles - 1].y;  // (the scan launch wrote the ranges)
        if (EXACT && cam.cull) {  // (the global-atomic path, > MAX_LDS_TILES tiles) the culled totals' prefix
            const uint32_t b = blockIdx.x, nb = gridDim.x;
            uint32_t cpre = 0, call = 0;
            for (uint32_t k = tid; k < nb; k += DUP_T) {
                const uint32_t c = geo.wgcull[k];
                call += c;
                cpre += k < b ? c : 0u;
            }
            cpre = wave_sum_u32(cpre);
            call = wave_sum_u32(call);
            if (lane == 0) {
                s_cred[0][w] = cpre;
                s_cred[1][w] = call;
            }
            __syncthreads();
            cpre = call = 0;
#pragma unroll
            for (int k = 0; k < DUP_T / 64; k++) {
                cpre += s_cred[0][k];
                call += s_cred[1][k];
            }
            ctail = geo.counters[0] - call + cpre;
        }
    }
    uint32_t tsum = 0, tmax = 0, cg[DUP_G], csum = 0;
#pragma unroll
    for (int g = 0; g < DUP_G; g++) {
        tsum += t[g];
        tmax = max(tmax, t[g]);
        cg[g] = (EXACT && cam.cull && t[g]) ? culled_below(r[g].w, t[g]) : 0u;
        csum += cg[g];
        const int q = DUP_G * tid + g;
        if (t[g]) {
            s_x0[q] = r[g].x & 0xFFFFu;
            s_y0[q] = r[g].x >> 16;
            s_w[q] = (r[g].y & 0xFFFFu) - (r[g].x & 0xFFFFu);
            s_depth[q] = r[g].z;
            s_live[q] = r[g].w;
        }
    }
    uint32_t incl = wave_incl_scan(tsum);
    const uint32_t cincl = (EXACT && cam.cull) ? wave_incl_scan(csum) : 0u;
    tmax = wave_max_u32(tmax);
    __syncthreads();  // (wsum is also tile_plan's scratch)
    if (lane == 63) {
        wsum[w] = incl;
        if (EXACT) s_cws[w] = cincl;
    }
    if (lane == 0) s_tmax[w] = tmax;
    __syncthreads();
    uint32_t run = incl - tsum, crun = ctail + cincl - csum;
    for (int k = 0; k < w; k++) {
        run += wsum[k];
        if (EXACT) crun += s_cws[k];
    }
#pragma unroll
    for (int k = 0; k < DUP_T / 64; k++) tmax = max(tmax, s_tmax[k]);
    uint32_t cx[DUP_G];  // (EXACT) the Gaussians' first slots in point_list's culled tail
#pragma unroll
    for (int g = 0; g < DUP_G; g++) {  // Gaussian order: the workgroup-local instance offsets of preprocess
        const uint32_t off = base + run;
        if (i0 + g < P) geo.offsets[i0 + g] = off;
        if (!EXACT && off + t[g] > ltot)  // padding tail: the owner of each rect slot >= L
            for (uint32_t u = max(off, ltot); u < off + t[g]; u++) point_list[u] = (uint64_t)(i0 + g);
        run += t[g];
        s_incl[DUP_G * tid + g] = run;
        cx[g] = crun;
        if (EXACT) s_cx[DUP_G * tid + g] = crun;  // (read by the load-balanced path)
        crun += cg[g];
    }
    if (tmax <= (uint32_t)GSR_DUP_LOOP_MAX) {
        // few tiles per Gaussian in this row (config 3: at most 4; mapping duplicate 50.4 -> 48.1 us at 16 or
        // 64, tracking 13.4 -> 11.9 at 8): every lane places its own Gaussians'
        // instances (<= GSR_DUP_LOOP_MAX loop trips) instead of one binary search over the row's
        // inclusive sums per instance; the slots within a tile bucket still come from the LDS cursors
        // (the bucket order is the sort's input, any order)
#pragma unroll
        for (int g = 0; g < DUP_G; g++) {
            const uint32_t x0 = r[g].x & 0xFFFFu, y0 = r[g].x >> 16, wdt = (r[g].y & 0xFFFFu) - x0;
            const uint32_t gi = (uint32_t)(i0 + g);
            uint32_t ct = cx[g];
            for (uint32_t k = 0; k < t[g]; k++) {
                if (!tile_live(r[g].w, k)) {  // culled (Camera::cull): not in the bucket (EXACT: in the tail)
                    if (EXACT) point_list[ct++] = (uint64_t)gi;
                    continue;
                }
                const uint32_t tile = (y0 + k / wdt) * (uint32_t)cam.gx + x0 + k % wdt;
                const uint32_t pos = LDS_HIST ? atomicAdd(&s_cur[tile], 1u)
                                              : ranges[tile].x + atomicAdd(&cursor[tile * TILE_CTR_STRIDE], 1u);
                keys[pos] = ((uint64_t)r[g].z << 32) | (uint64_t)gi;
            }
        }
        return;
    }
    __syncthreads();
    const uint32_t total = s_incl[ROW - 1];
    for (uint32_t e = tid; e < total; e += DUP_T) {
        int lo = 0, hi = ROW - 1;
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if (s_incl[mid] > e) hi = mid; else lo = mid + 1;
        }
        const uint32_t local = e - ((lo == 0) ? 0u : s_incl[lo - 1]);
        if (!tile_live(s_live[lo], local)) {  // culled (Camera::cull): not in the bucket (EXACT: in the tail)
            if (EXACT)
                point_list[s_cx[lo] + culled_below(s_live[lo], local)] = (uint64_t)(blockIdx.x * ROW + lo);
            continue;
        }
        const uint32_t wdt = s_w[lo];
        const uint32_t tile = (s_y0[lo] + local / wdt) * (uint32_t)cam.gx + s_x0[lo] + local % wdt;
        const uint32_t pos = LDS_HIST ? atomicAdd(&s_cur[tile], 1u)
                                      : ranges[tile].x + atomicAdd(&cursor[tile * TILE_CTR_STRIDE], 1u);
        const uint32_t gi = blockIdx.x * ROW + lo;
        keys[pos] = ((uint64_t)s_depth[lo] << 32) | (uint64_t)gi;
    }
}
// EXACT instantiations: at most 80 VGPRs (6 waves per SIMD), three 512-lane workgroups per CU, so config 3's 586
// count-matrix rows run in one dispatch round on 256 CUs (that bookkeeping took the kernel to 88 VGPRs: two
// workgroups per CU, a second round, 10.8 -> 14.5 us); the padding ones stay at 72-79 VGPRs by themselves
template <bool LDS_HIST, int DUP_G, bool CLK, bool EXACT>
__global__ void __launch_bounds__(DUP_T) __attribute__((amdgpu_waves_per_eu(6, 8)))
duplicate_bucket_kernel(Camera cam, int P, GeomPtrs geo, uint2* __restrict__ ranges, const uint32_t* __restrict__ tot,
                        uint32_t* __restrict__ cursor, int ntiles, uint64_t* __restrict__ keys,
                        uint64_t* __restrict__ point_list, SpecGuard guard, uint32_t sort_cap,
                        uint32_t* __restrict__ status, unsigned long long* clk) {
    extern __shared__ uint32_t s_cur[];
    if (cam.gate.off()) {
        dup_gate_off_snap(cam, geo);
        return;
    }
    if constexpr (CLK) kclock_begin(clk);
    duplicate_bucket_body<LDS_HIST, DUP_G, EXACT>(cam, P, geo, ranges, tot, cursor, ntiles, keys, point_list, guard,
                                                  sort_cap, status, s_cur);
    if constexpr (CLK) kclock_end(clk);
}
// The exact-tail form (the dynamic forward) needs ~88 VGPRs: at the 80-VGPR cap above it spills 80 B per
// lane; GSR_DUP_EXACT_WAVES sets its own occupancy target
#ifndef GSR_DUP_EXACT_WAVES
#define GSR_DUP_EXACT_WAVES 6
#endif
template <bool LDS_HIST, int DUP_G, bool CLK>
__global__ void __launch_bounds__(DUP_T) __attribute__((amdgpu_waves_per_eu(GSR_DUP_EXACT_WAVES, 8)))
duplicate_bucket_exact_kernel(Camera cam, int P, GeomPtrs geo, uint2* __restrict__ ranges,
                              const uint32_t* __restrict__ tot, uint32_t* __restrict__ cursor, int ntiles,
                              uint64_t* __restrict__ keys, uint64_t* __restrict__ point_list, SpecGuard guard,
                              uint32_t sort_cap, uint32_t* __restrict__ status, unsigned long long* clk) {
    extern __shared__ uint32_t s_cur[];
    if (cam.gate.off()) {
        dup_gate_off_snap(cam, geo);
        return;
    }
    if constexpr (CLK) kclock_begin(clk);
    duplicate_bucket_body<LDS_HIST, DUP_G, true>(cam, P, geo, ranges, tot, cursor, ntiles, keys, point_list, guard,
                                                 sort_cap, status, s_cur);
    if constexpr (CLK) kclock_end(clk);
}

// The 16 forms: the exact tail is a kernel of its own (its occupancy target), not a template argument
struct PickDuplicateBucket {
    template <bool LDS_HIST, bool G2, bool CLK, bool EXACT>
    auto operator()() const {
        if constexpr (EXACT) return &duplicate_bucket_exact_kernel<LDS_HIST, G2 ? 2 : 1, CLK>;
        else return &duplicate_bucket_kernel<LDS_HIST, G2 ? 2 : 1, CLK, false>;
    }
};

hipError_t launch_duplicate_bucket(const Camera& cam, int P, GeomPtrs geo, uint2* ranges, const uint32_t* tot,
                                   uint32_t* cursor, bool lds_hist, int ntiles, uint64_t* keys, uint64_t* point_list,
                                   int nb, SpecGuard guard, uint32_t* status, hipStream_t s, unsigned long long* clk) {
    if (nb == 0) return hipSuccess;
    const bool g2 = cam.pre_shift == 10;  // rows of 1024: two Gaussians per lane; of 512: one
    const auto k = dispatch_bools(PickDuplicateBucket{}, lds_hist, g2, clk != nullptr, cam.tail_exact != 0);
    hipLaunchKernelGGL(k, dim3(nb), dim3(DUP_T), lds_hist ? sizeof(uint32_t) * ntiles : 0, s, cam, P, geo, ranges,
                       tot, cursor, ntiles, keys, point_list, guard, (uint32_t)TILE_SORT_CAP, status, clk);
    return hipGetLastError();
}

}  // namespace gsr
