// gsr_radix.hip -- the forward's fallback binning: the reference's own scheme, a global sort of (tile, depth)
// keys (duplicateWithKeys and cub's SortPairs, rasterizer_impl.cu:70-111, 301-309).
// It runs in the dynamic forward only, after the host has read the counters (Forward::wait_and_finish ->
// radix_binning, gsr_capi.hip): when a tile's list is longer than TILE_SORT_CAP, the longest the render's
// per-tile sort handles, or when GSR_FORCE_RADIX is set (then the bucketed duplicate is not enqueued at all).
// The static forward never takes it: there a list that long is an overflow in the status row.
//   duplicate   a workgroup emits the instances of its row of Gaussians with consecutive lanes on
//               consecutive instances (binary search in LDS), so the key writes are coalesced
//   radix sort  stable 8-bit LSD passes, wave64 ballot match ranking (no atomics), values = instance index
//   gather      point_list = the Gaussian ids in sorted order
// The tile ranges are the count scan's (gsr_binning.hip), and the render gets no keys and skips its sort.
#include "gsr_launch.h"
#include "gsr_layout.h"
#include "gsr_math.h"
#include "gsr_wave.h"

namespace gsr {

// -------------------------------------------------------------- duplicate --
__global__ void __launch_bounds__(PRE_BLOCK)
duplicate_kernel(Camera cam, int P, GeomPtrs geo, uint64_t* __restrict__ keys, uint32_t* __restrict__ gid) {
    __shared__ uint32_t s_incl[PRE_BLOCK];   // inclusive scan of tiles touched
    __shared__ uint32_t s_x0[PRE_BLOCK], s_y0[PRE_BLOCK], s_w[PRE_BLOCK], s_depth[PRE_BLOCK], s_live[PRE_BLOCK];
    __shared__ uint32_t wsum[PRE_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, R = (int)blockDim.x;  // R = 1 << pre_shift
    const int i = (blockIdx.x << cam.pre_shift) + tid;
    uint32_t t = (i < P) ? geo.tiles[i] : 0u;
    uint32_t incl = wave_incl_scan(t);
    if (lane == 63) wsum[w] = incl;
    if (t) {
        const uint4 r = geo.bin[i];  // (rect lo, rect hi, depth bits, tiles)
        s_x0[tid] = r.x & 0xFFFFu;
        s_y0[tid] = r.x >> 16;
        s_w[tid] = (r.y & 0xFFFFu) - (r.x & 0xFFFFu);
        s_depth[tid] = r.z;
        s_live[tid] = r.w;
    }
    __syncthreads();
    uint32_t woff = 0;
    for (int k = 0; k < w; k++) woff += wsum[k];
    incl += woff;
    s_incl[tid] = incl;
    const uint32_t base = geo.blocksums[blockIdx.x];  // exclusive scan of workgroup totals
    if (i < P) geo.offsets[i] = base + incl - t;
    __syncthreads();
    const uint32_t total = s_incl[R - 1];
    for (uint32_t e = tid; e < total; e += R) {
        // owner j: first Gaussian whose inclusive sum exceeds e
        int lo = 0, hi = R - 1;
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if (s_incl[mid] > e) hi = mid; else lo = mid + 1;
        }
        const uint32_t start = (lo == 0) ? 0u : s_incl[lo - 1];
        const uint32_t local = e - start;
        const uint32_t wdt = s_w[lo];
        const uint32_t ty = s_y0[lo] + local / wdt;
        const uint32_t tx = s_x0[lo] + local % wdt;
        const uint32_t u = base + e;
        const uint32_t gi = (blockIdx.x << cam.pre_shift) + lo;
        // a culled instance (Camera::cull) sorts behind every tile (tile id gx * gy, within the sorted bits), so
        // the live ones take the positions the culled tile counts' ranges give them
        const uint32_t tkey = tile_live(s_live[lo], local) ? ty * (uint32_t)cam.gx + tx : (uint32_t)(cam.gx * cam.gy);
        keys[u] = ((uint64_t)tkey << 32) | (uint64_t)s_depth[lo];
        gid[u] = gi;
    }
}

hipError_t launch_duplicate(const Camera& cam, int P, GeomPtrs geo, uint64_t* keys, uint32_t* gid,
                            int nb, hipStream_t s) {
    if (nb == 0) return hipSuccess;
    hipLaunchKernelGGL(duplicate_kernel, dim3(nb), dim3(1 << cam.pre_shift), 0, s, cam, P, geo, keys, gid);
    return hipGetLastError();
}

// ------------------------------------------------------------- radix sort --
// Each workgroup owns SORT_TILE consecutive keys; wave w owns the w-th quarter
// in 8 slots of 64 lanes, so (wave, slot, lane) order == key order (stable).
__global__ void __launch_bounds__(SORT_THREADS)
radix_hist_kernel(const uint64_t* __restrict__ keys, uint32_t n, int shift, uint32_t* __restrict__ hist, int nsb) {
    __shared__ uint32_t wcnt[SORT_THREADS / 64][RADIX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int k = tid; k < (SORT_THREADS / 64) * RADIX; k += SORT_THREADS) (&wcnt[0][0])[k] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * SORT_TILE + w * (SORT_TILE / 4);
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int s = 0; s < SORT_ITEMS; s++) {
        const uint32_t idx = base + s * 64 + lane;
        const bool valid = idx < n;
        const uint32_t d = valid ? (uint32_t)(keys[idx] >> shift) & (RADIX - 1) : 0u;
        const uint64_t m = wave_match8(d, valid);
        if (valid && (m & lt) == 0) wcnt[w][d] += (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < SORT_THREADS / 64; k++) c += wcnt[k][tid];
    hist[(size_t)tid * nsb + blockIdx.x] = c;
}

// Per-digit exclusive scan of the [digit][block] histogram rows: workgroup d
// scans row d in place and writes the digit total (no single-workgroup
// bottleneck over RADIX * nsb entries).
__global__ void __launch_bounds__(256) radix_rowscan_kernel(uint32_t* __restrict__ hist, int nsb,
                                                            uint32_t* __restrict__ digit_total) {
    __shared__ uint32_t wsums[4];
    __shared__ uint32_t s_carry;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t* row = hist + (size_t)blockIdx.x * nsb;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nsb; base += 256) {
        const int i = base + tid;
        const uint32_t x = (i < nsb) ? row[i] : 0u;
        const uint32_t incl = wave_incl_scan(x);
        if (lane == 63) wsums[w] = incl;
        __syncthreads();
        uint32_t off = s_carry;
        for (int k = 0; k < w; k++) off += wsums[k];
        if (i < nsb) row[i] = off + incl - x;
        __syncthreads();
        if (tid == 255) s_carry = off + incl;
        __syncthreads();
    }
    if (tid == 0) digit_total[blockIdx.x] = s_carry;
}

__global__ void __launch_bounds__(SORT_THREADS)
radix_scatter_kernel(const uint64_t* __restrict__ kin, const uint32_t* __restrict__ vin, uint64_t* __restrict__ kout,
                     uint32_t* __restrict__ vout, uint32_t n, int shift, const uint32_t* __restrict__ hist, int nsb,
                     const uint32_t* __restrict__ digit_total) {
    __shared__ uint32_t wcnt[SORT_THREADS / 64][RADIX];
    __shared__ uint32_t s_dsum[SORT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int k = tid; k < (SORT_THREADS / 64) * RADIX; k += SORT_THREADS) (&wcnt[0][0])[k] = 0;
    // exclusive scan of the 256 digit totals -> global base of each digit
    const uint32_t dt = digit_total[tid];
    const uint32_t dincl = wave_incl_scan(dt);
    if (lane == 63) s_dsum[w] = dincl;
    __syncthreads();
    uint32_t dbase = dincl - dt;
    for (int k = 0; k < w; k++) dbase += s_dsum[k];
    const uint32_t base = blockIdx.x * SORT_TILE + w * (SORT_TILE / 4);
    const uint64_t lt = (1ull << lane) - 1ull;
    uint64_t key[SORT_ITEMS];
    uint32_t val[SORT_ITEMS], rank[SORT_ITEMS], dig[SORT_ITEMS];
#pragma unroll
    for (int s = 0; s < SORT_ITEMS; s++) {
        const uint32_t idx = base + s * 64 + lane;
        const bool valid = idx < n;
        key[s] = valid ? kin[idx] : 0ull;
        val[s] = valid ? (vin ? vin[idx] : idx) : 0u;
        const uint32_t d = (uint32_t)(key[s] >> shift) & (RADIX - 1);
        dig[s] = d;
        const uint64_t m = wave_match8(d, valid);
        uint32_t prev = 0;
        if (valid) prev = wcnt[w][d];
        rank[s] = prev + (uint32_t)__popcll(m & lt);
        if (valid && (m & lt) == 0) wcnt[w][d] = prev + (uint32_t)__popcll(m);
    }
    __syncthreads();
    {
        const uint32_t c0 = wcnt[0][tid], c1 = wcnt[1][tid], c2 = wcnt[2][tid];
        const uint32_t g = dbase + hist[(size_t)tid * nsb + blockIdx.x];
        __syncthreads();
        wcnt[0][tid] = g;
        wcnt[1][tid] = g + c0;
        wcnt[2][tid] = g + c0 + c1;
        wcnt[3][tid] = g + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SORT_ITEMS; s++) {
        const uint32_t idx = base + s * 64 + lane;
        if (idx < n) {
            const uint32_t pos = wcnt[w][dig[s]] + rank[s];
            kout[pos] = key[s];
            vout[pos] = val[s];
        }
    }
}

hipError_t launch_radix_sort(uint64_t* keys[2], uint32_t* vals[2], uint32_t* hist, uint32_t n, int nsb, int npass,
                             hipStream_t s) {
    uint32_t* digit_total = hist + (size_t)RADIX * nsb;
    for (int p = 0; p < npass; p++) {
        const int in = p & 1, out = in ^ 1;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(nsb), dim3(SORT_THREADS), 0, s, keys[in], n, 8 * p, hist, nsb);
        hipLaunchKernelGGL(radix_rowscan_kernel, dim3(RADIX), dim3(256), 0, s, hist, nsb, digit_total);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nsb), dim3(SORT_THREADS), 0, s, keys[in],
                           p == 0 ? (const uint32_t*)nullptr : vals[in], keys[out], vals[out], n, 8 * p, hist, nsb,
                           digit_total);
    }
    return hipGetLastError();
}

// ----------------------------------------------------------------- gather --
// Gaussian ids of the radix-sorted instances (values are unsorted instance indices).
__global__ void gather_ids_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ gid,
                                  uint64_t* __restrict__ point_list, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) point_list[k] = (PointEntry)gid[vals[k]];
}

hipError_t launch_gather_ids(const uint32_t* vals, const uint32_t* gid, uint64_t* point_list, uint32_t n,
                             hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_ids_kernel, dim3((n + 255) / 256), dim3(256), 0, s, vals, gid, point_list, n);
    return hipGetLastError();
}

}  // namespace gsr
