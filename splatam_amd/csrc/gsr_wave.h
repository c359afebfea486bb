// gsr_wave.h -- wave64 and workgroup building blocks of the kernels: lane scans and row lists, the
// agent-scope hand-off with its arrival counters, DPP / permlane reductions and the streaming loads and
// stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

// inclusive scan over the 64 lanes: six DPP adds (row_shr 1 / 2 / 4 / 8 with bank masks: the in-row prefix; row_bcast 15 / 31 carry it across
// rows) instead of six lane shuffles through the LDS crossbar
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xe, true);   // row_shr:4 (banks 1-3)
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xc, true);   // row_shr:8 (banks 2-3)
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 (rows 1, 3)
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 (rows 2, 3)
    return v;
}
// sum and maximum over the 64 lanes, in every lane (xor butterflies)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m));
    return v;
}
// number of set bits of `mask` below this lane (v_mbcnt_lo / hi)
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Ordered list of the batch entries whose quadrant mask has bit `w` (one wave
// builds its own list; ballot + popcount compaction, order preserved).
__device__ __forceinline__ int build_wave_list(const uint8_t* s_mask, int cnt, int w, int jmin, uint16_t* list) {
    const int lane = __lane_id();
    const uint64_t lt = (1ull << lane) - 1ull;
    int n = 0;
    for (int c = 0; c < cnt; c += 64) {
        const int j = c + lane;
        const bool bit = j < cnt && j >= jmin && ((s_mask[j] >> w) & 1u);
        const uint64_t bal = __ballot(bit);
        if (bit) list[n + __popcll(bal & lt)] = (uint16_t)j;
        n += __popcll(bal);
    }
    return n;
}

// The four ordered lists of a wave's 16-lane rows: list[r] gets the batch
// entries whose 16-bit block mask has bit 4w + r (ballot + popcount
// compaction, order preserved), skipping entries j < jmin[r].  Every list is
// then padded with `pad` (the index of a staged dummy entry that never blends)
// up to the returned length: the longest list rounded up to 4, so the rows of
// a wave step through their lists in lockstep with no validity tests.
// jmul scales the stored j (the walk may take it as an LDS byte offset; j * jmul must stay below 2^16).
template <typename MaskOf>
__device__ __forceinline__ int build_row_lists_by(MaskOf mask_of, int cnt, int w, const int (&jmin)[4],
                                                  uint16_t* list, int stride, uint16_t pad, uint32_t jmul = 1u) {
    const int lane = __lane_id();
    int n[4] = {0, 0, 0, 0};
    for (int c = 0; c < cnt; c += 64) {
        const int j = c + lane;
        const uint32_t m = j < cnt ? (mask_of(j) >> (4 * w)) & 0xFu : 0u;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // the row's lanes as an SGPR mask: its lane prefix by v_mbcnt, the store predicated on it
            const uint64_t bal = __builtin_amdgcn_uicmp((m >> r) & 1u, 0u, 33 /* ne */) &
                                 __builtin_amdgcn_sicmp(j, jmin[r], 39 /* sge */);
            if (__builtin_amdgcn_inverse_ballot_w64(bal))
                list[r * stride + n[r] + (int)lanes_below(bal)] = (uint16_t)((uint32_t)j * jmul);
            n[r] += __popcll(bal);
        }
    }
    const int len = (max(max(n[0], n[1]), max(n[2], n[3])) + 3) & ~3;
#pragma unroll
    for (int r = 0; r < 4; r++)
        for (int p = n[r] + lane; p < len; p += 64) list[r * stride + p] = pad;
    return len;
}
__device__ __forceinline__ int build_row_lists(const uint16_t* s_mask, int cnt, int w, const int (&jmin)[4],
                                               uint16_t* list, int stride, uint16_t pad, uint32_t jmul = 1u) {
    return build_row_lists_by([&](int j) { return (uint32_t)s_mask[j]; }, cnt, w, jmin, list, stride, pad, jmul);
}

// Four consecutive entries of this lane's (padded) row list, per lane (VGPR).
struct RowGroup4 {
    int j[4];
};
__device__ __forceinline__ RowGroup4 load_row_group4(const uint16_t* row_list, int i) {
    const uint2 q = *reinterpret_cast<const uint2*>(&row_list[i]);
    RowGroup4 g;
    g.j[0] = (int)(q.x & 0xFFFFu);
    g.j[1] = (int)(q.x >> 16);
    g.j[2] = (int)(q.y & 0xFFFFu);
    g.j[3] = (int)(q.y >> 16);
    return g;
}

// Per-wave row lists of one batch: row r of wave w (tile block b = 4w + r) lists the entries j
// (< cnt) whose block mask has bit b and that lie before the block's last contributor (j >=
// jmin[r]), as (j | slot << 16) with slot = the entry's slot for block b; every wave also forms
// the batch's slot bases (exclusive scan of the masks' popcounts, redundantly per wave) and
// returns cnt = the longest prefix of the cmax staged entries whose slots fit in `budget`.
// Lists are padded to a common multiple of 4 with `pad`.  Wave 0 publishes the bases.
struct SlotLists {
    int len, cnt;
};
// jmul / smul scale the stored j and slot (the walk may take them as LDS byte offsets: j * record
// size, slot * slot size; both must stay below 2^16).
__device__ __forceinline__ SlotLists build_row_slot_lists(const uint16_t* s_mask, uint16_t* s_base, int cmax,
                                                         int budget, int w, const int (&jmin)[4], uint32_t* list,
                                                         int stride, uint32_t pad, uint32_t jmul = 1u,
                                                         uint32_t smul = 1u) {
    const int lane = __lane_id();
    const uint32_t below_w = (1u << (4 * w)) - 1u;  // blocks of the waves before this one
    int n[4] = {0, 0, 0, 0};
    uint32_t carry = 0;
    int cnt = 0;
    for (int c = 0; c < cmax; c += 64) {
        const int j = c + lane;
        const uint32_t mf = j < cmax ? (uint32_t)s_mask[j] : 0u;
        const uint32_t pc = __popc(mf);
        // inclusive prefix of the popcounts over the batch (DPP scan), the chunk total from lane 63
        const uint32_t incl = carry + wave_incl_scan(pc);
        const uint32_t base = incl - pc;
        const uint64_t fits = __builtin_amdgcn_sicmp(j, cmax, 40 /* slt */) &
                              __builtin_amdgcn_uicmp(incl, (uint32_t)budget, 37 /* ule */);
        cnt += __popcll(fits);
        carry = __builtin_amdgcn_readlane(incl, 63);
        if (w == 0 && __builtin_amdgcn_inverse_ballot_w64(fits)) s_base[j] = (uint16_t)base;
        const uint32_t m = (mf >> (4 * w)) & 0xFu;
        // the entry's word for the wave's first block; block r adds the slots of blocks r' < r it reaches
        const uint32_t w0 = __umul24((uint32_t)j, jmul) | (__umul24(base + __popc(mf & below_w), smul) << 16);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // compare masks straight from v_cmp (a __ballot of a combined bool costs a select and a compare
            // more per row)
            const uint64_t bal = __builtin_amdgcn_uicmp((m >> r) & 1u, 0u, 33 /* ne */) &
                                 __builtin_amdgcn_sicmp(j, jmin[r], 39 /* sge */) & fits;
            if (__builtin_amdgcn_inverse_ballot_w64(bal))
                list[r * stride + n[r] + (int)lanes_below(bal)] = w0 + (__umul24(__popc(m & ((1u << r) - 1u)), smul) << 16);
            n[r] += __popcll(bal);
        }
    }
    const int len = (max(max(n[0], n[1]), max(n[2], n[3])) + 3) & ~3;
#pragma unroll
    for (int r = 0; r < 4; r++)
        for (int p = n[r] + lane; p < len; p += 64) list[r * stride + p] = pad;
    return {len, cnt};
}
// Four consecutive (j | slot << 16) words of this lane's row list.
__device__ __forceinline__ uint4 load_slot_group4(const uint32_t* row_list, int i) {
    return *reinterpret_cast<const uint4*>(&row_list[i]);
}

// Cross-workgroup hand-off inside one launch without a release fence (an agent-
// scope release is an L2 writeback per workgroup on this multi-XCD part): the
// producers publish with agent-scope atomic stores (written through to the
// coherence point), wait for them (vmcnt 0), and count themselves done with one
// relaxed atomic; the last workgroup to arrive reads with agent-scope atomic
// loads and resets the counter for the next launch.
__device__ __forceinline__ void st_agent(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_agent(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The last workgroup's fixed-order gather of per-workgroup partials: thread t adds values
// k < N of part[stride * b + k] for b = t, t + nt, t + 2 nt, ... in that order -- the same
// sums, bit for bit, as the plain loop (v starts at +0, and the out-of-range slots add +0),
// but CH partials' loads are in flight per memory round trip (the plain loop waited for each
// agent-scope load before issuing the next iteration's).
template <int N, int CH>
__device__ __forceinline__ void gather_partials(const float* part, int stride, int nb, int t, int nt,
                                                float (&v)[N]) {
    for (int b0 = t; b0 < nb; b0 += CH * nt) {
        float buf[CH][N];
#pragma unroll
        for (int u = 0; u < CH; u++) {
            const int b = b0 + u * nt;
#pragma unroll
            for (int k = 0; k < N; k++) buf[u][k] = b < nb ? ld_agent(part + (size_t)stride * b + k) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CH; u++)
#pragma unroll
            for (int k = 0; k < N; k++) v[k] += buf[u][k];
    }
}
// Same for large grids: 16 group counters (workgroup id mod 16, 64 B apart)
// and a top counter, so no single address takes more than ~nb/16 atomics
// (same-address atomics serialise: one counter for 1024 workgroups cost
// ~15 us).  ctr: ARRIVE_GROUPED_WORDS words, zero before the first launch.
constexpr int ARRIVE_STRIDE = 16;
constexpr int ARRIVE_GROUPED_WORDS = 17 * ARRIVE_STRIDE;
// Layout of every reduction scratch (include/gsr_glue.h): the arrival counters are its first
// ARRIVE_GROUPED_WORDS words, whatever the grid, and the partials follow.  Only the counters must
// stay zero between launches (each launch writes the partials it reads), so users with different
// grids can share one buffer: no user's partials ever land on another's counters.
__host__ __device__ __forceinline__ uint32_t* scratch_counters(float* scratch) {
    return reinterpret_cast<uint32_t*>(scratch);
}
__host__ __device__ __forceinline__ float* scratch_partials(float* scratch) { return scratch + ARRIVE_GROUPED_WORDS; }
__device__ __forceinline__ bool last_block_arrive_grouped(uint32_t* ctr) {
    __shared__ uint32_t s_last2;
    __builtin_amdgcn_s_waitcnt(0x0F70);  // s_waitcnt vmcnt(0)
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nb = gridDim.x * gridDim.y * gridDim.z;
        const uint32_t b = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, g = b & 15u;
        const uint32_t ngroups = nb < 16u ? nb : 16u, gsize = nb / 16u + (g < nb % 16u ? 1u : 0u);
        uint32_t* gc = ctr + ARRIVE_STRIDE * (1 + g);
        uint32_t last = 0;
        if (__hip_atomic_fetch_add(gc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1) {
            __hip_atomic_store(gc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngroups - 1) {
                __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = 1;
            }
        }
        s_last2 = last;
    }
    __syncthreads();
    return s_last2 != 0u;
}

// Every thread of the workgroup calls this after its st_agent stores; true in
// the last workgroup of the grid to arrive (then *counter is back to 0).
__device__ __forceinline__ bool last_block_arrive(uint32_t* counter) {
    __shared__ uint32_t s_last;
    __builtin_amdgcn_s_waitcnt(0x0F70);  // s_waitcnt vmcnt(0): this thread's stores have landed
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nb = gridDim.x * gridDim.y * gridDim.z;
        const uint32_t old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == nb - 1 ? 1u : 0u;
        if (old == nb - 1) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return s_last != 0u;
}

// --------------------------------------------------------- wave64 helpers --
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Sum over each 16-lane row; every lane of the row receives the row total.
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x124>(v);  // row_ror:4
    v += dpp_mov<0x128>(v);  // row_ror:8
    return v;
}

// v_permlane32_swap: lanes 0-31 <- a(l)+a(l+32), lanes 32-63 <- b(l-32)+b(l)
__device__ __forceinline__ float swapsum32(float a, float b) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// v_permlane16_swap: within each 32-lane half, row0 <- a.r0+a.r1, row1 <- b.r0+b.r1
__device__ __forceinline__ float swapsum16(float a, float b) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Transposed wave reduction of 9 values: ~30 VALU instead of 9 full
// butterflies.  On return, for row = lane/16:
//   r0 row {0,1,2,3} holds the wave totals of v{0,2,1,3}
//   r1 row {0,1,2,3} holds the wave totals of v{4,6,5,7}
//   r8 row 0 holds the wave total of v8
__device__ __forceinline__ void wave_reduce9(const float v[9], float& r0, float& r1, float& r8) {
    float s01 = swapsum32(v[0], v[1]);
    float s23 = swapsum32(v[2], v[3]);
    float s45 = swapsum32(v[4], v[5]);
    float s67 = swapsum32(v[6], v[7]);
    float s8 = swapsum32(v[8], 0.f);
    float t0 = swapsum16(s01, s23);
    float t1 = swapsum16(s45, s67);
    float t2 = swapsum16(s8, 0.f);
    r0 = row16_sum(t0);
    r1 = row16_sum(t1);
    r8 = row16_sum(t2);
}
__device__ __forceinline__ int reduce9_slot_r0(int row) { return (row == 0) ? 0 : (row == 1 ? 2 : (row == 2 ? 1 : 3)); }

// Four consecutive entries of a wave's quadrant list as wave-uniform (SGPR)
// indices; entries past n repeat the first one and are flagged invalid.
struct Group4 {
    int j[4];
    bool valid[4];
};
__device__ __forceinline__ Group4 load_group4(const uint16_t* list, int i, int n) {
    const uint2 q = *reinterpret_cast<const uint2*>(&list[i]);
    const uint32_t q0 = __builtin_amdgcn_readfirstlane(q.x), q1 = __builtin_amdgcn_readfirstlane(q.y);
    Group4 g;
    g.j[0] = (int)(q0 & 0xFFFFu);
    g.j[1] = (int)(q0 >> 16);
    g.j[2] = (int)(q1 & 0xFFFFu);
    g.j[3] = (int)(q1 >> 16);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        g.valid[k] = i + k < n;
        if (!g.valid[k]) g.j[k] = g.j[0];
    }
    return g;
}

// Transposed reduction of 4 items x 9 values (v[item*9 + q]) over the 64 lanes:
// 18 permlane32 + 9 permlane16 swaps and 36 DPP adds (~2.5 VALU per value).
// On return row rho (= lane / 16) of r[q] holds, in all its 16 lanes, the wave
// total of value q of item rho.
__device__ __forceinline__ void wave_reduce4x9(const float (&v)[36], float (&r)[9]) {
    float r1[18];
#pragma unroll
    for (int n = 0; n < 18; n++) r1[n] = swapsum32(v[n], v[n + 18]);
#pragma unroll
    for (int m = 0; m < 9; m++) r[m] = row16_sum(swapsum16(r1[m], r1[m + 9]));
}

// Same for 2 items x 9 values (v[item*9 + q]).  On return, for row rho:
//   r[m] (m < 4) holds value q = m + 4*(rho & 1) of item rho >> 1,
//   r[4] holds value 8 of item rho >> 1 in rows 0 and 2 (rows 1, 3: zero).
__device__ __forceinline__ void wave_reduce2x9(const float (&v)[18], float (&r)[5]) {
    float r1[9];
#pragma unroll
    for (int q = 0; q < 9; q++) r1[q] = swapsum32(v[q], v[q + 9]);
#pragma unroll
    for (int m = 0; m < 4; m++) r[m] = row16_sum(swapsum16(r1[m], r1[m + 4]));
    r[4] = row16_sum(swapsum16(r1[8], 0.f));
}

// Transposed reduction of N values (N a multiple of 4) over the 64 lanes.
// On return row rho (= lane / 16) of r[m] (m < N/4) holds the wave total of
// v[m + rho * N / 4] in all 16 lanes of the row.
// Sums over each 16-lane row of 4 entries x NV values (v[e * NV + m], entry-major),
// transposed: a step pairs every lane with a partner differing in one lane class
// bit; the lane keeps one half of its values and adds the partner's copy of that
// half (2 selects + 1 DPP add per kept value), so each step halves what a lane
// holds.  Partners: row_ror:8 (lane ^ 8), row_half_mirror (i <-> 7 - i, which
// flips class bit 4), quad_perm [2,3,0,1] (^ 2), quad_perm [1,0,3,2] (^ 1).  The
// first two steps split the entries: lane class e = 2 (lane>>3 & 1) + (lane>>2 & 1)
// ends up with NV values of entry e; further transposed steps split m while the
// count stays even, plain DPP adds finish the rest.  Cost ~2.8 VALU per value
// against 4 for four plain DPP steps per value.
template <int NV>
struct RowReduce {
    static constexpr int V = 4 * NV;
    static constexpr int S = (V / 4) % 2 ? 2 : ((V / 8) % 2 ? 3 : 4);  // transposed steps (>= 2)
    static constexpr int R = V >> S;                                     // values per lane at the end
    // lanes that hold (and write) distinct results: class bits of the plain steps are 0
    static constexpr int WRITER_MASK = S == 2 ? 3 : (S == 3 ? 1 : 0);
};

template <int N, int CTRL>
__device__ __forceinline__ void row_tstep(const float* c, float* out, bool hi) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
        const float keep = hi ? c[i + N / 2] : c[i];
        const float send = hi ? c[i] : c[i + N / 2];
        out[i] = keep + dpp_mov<CTRL>(send);
    }
}

// The same step for partners in the other half of a 4-lane-bank pair (row_ror:8: banks
// {0,1} <-> {2,3}; row_half_mirror: banks {0,2} <-> {1,3}): two v_add_f32_dpp whose
// bank masks write complementary lane halves -- lanes of the low half add the pair's c[i],
// lanes of the high half c[i + N/2] -- instead of two selects and one DPP add per value.
// Each pair is its own asm block and starts with s_nop 1: the VALU-write -> DPP-read hazard of its
// inputs needs 2 wait states, and the compiler, which does not see the DPP inside, may schedule the
// VALU that writes an input right before any of the blocks (a single s_nop ahead of the first block
// once let a select land between two blocks and the DPP read the stale register: the Fisher kernel's
// opacity column at 4 waves/SIMD).  Requires full EXEC.
template <int N>
__device__ __forceinline__ void row_tstep_ror8(const float* c, float* out) {
    static_assert(N % 2 == 0, "even value count");
#pragma unroll
    for (int i = 0; i < N / 2; i++)
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
                     "v_add_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xc"
                     : "=&v"(out[i]) : "v"(c[i]), "v"(c[i + N / 2]));
}
template <int N>
__device__ __forceinline__ void row_tstep_mirror(const float* c, float* out) {
    static_assert(N % 2 == 0, "even value count");
#pragma unroll
    for (int i = 0; i < N / 2; i++)
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %1, %1 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
                     "v_add_f32_dpp %0, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xa"
                     : "=&v"(out[i]) : "v"(c[i]), "v"(c[i + N / 2]));
}

// r[i] = row total of value (entry row_entry(lane), m = row_m0<NV>(lane) + i)
template <int NV>
__device__ __forceinline__ void row_reduce(const float (&v)[4 * NV], float (&r)[RowReduce<NV>::R], int lane) {
    using RR = RowReduce<NV>;
    constexpr int V = RR::V;
    float a[V / 2], b[V / 4];
    row_tstep_ror8<V>(v, a);                    // row_ror:8, bank-masked pair adds
    row_tstep_mirror<V / 2>(a, b);              // row_half_mirror, bank-masked pair adds
    if constexpr (RR::S == 2) {
#pragma unroll
        for (int i = 0; i < RR::R; i++) {
            float t = b[i] + dpp_mov<0x4E>(b[i]);
            r[i] = t + dpp_mov<0xB1>(t);
        }
    } else if constexpr (RR::S == 3) {
        float c[V / 8];
        row_tstep<V / 4, 0x4E>(b, c, lane & 2);
#pragma unroll
        for (int i = 0; i < RR::R; i++) r[i] = c[i] + dpp_mov<0xB1>(c[i]);
    } else {
        float c[V / 8];
        row_tstep<V / 4, 0x4E>(b, c, lane & 2);
        row_tstep<V / 8, 0xB1>(c, r, lane & 1);
    }
    // the totals formed here, in every lane: otherwise the compiler sinks the plain steps' adds into the
    // caller's writer-lane branch, where a DPP read of a disabled lane is invalid, so each step becomes
    // v_mov_b32_dpp (outside) + v_add_f32 (inside) instead of one v_add_f32_dpp (same operands, same sum:
    // 51 -> 45 reduction VALU per walk step, profiles/r8h_ab_pk_reduce.txt)
#pragma unroll
    for (int i = 0; i < RR::R; i++) asm volatile("" : "+v"(r[i]));
}
__device__ __forceinline__ int row_entry(int lane) { return 2 * ((lane >> 3) & 1) + ((lane >> 2) & 1); }
template <int NV>
__device__ __forceinline__ int row_m0(int lane) {
    using RR = RowReduce<NV>;
    int m0 = 0;
    if (RR::S >= 3 && (lane & 2)) m0 += NV / 2;
    if (RR::S >= 4 && (lane & 1)) m0 += NV / 4;
    return m0;
}

template <int N>
__device__ __forceinline__ void wave_reduce_n(const float (&v)[N], float (&r)[N / 4]) {
    static_assert(N % 4 == 0, "pad to a multiple of 4");
    float r1[N / 2];
#pragma unroll
    for (int n = 0; n < N / 2; n++) r1[n] = swapsum32(v[n], v[n + N / 2]);
#pragma unroll
    for (int m = 0; m < N / 4; m++) r[m] = row16_sum(swapsum16(r1[m], r1[m + N / 4]));
}

__device__ __forceinline__ int lane_id() { return __lane_id(); }

// Lanes of the wave whose 8-bit digit equals mine (valid lanes only).
__device__ __forceinline__ uint64_t wave_match8(uint32_t d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        uint64_t bal = __ballot(valid && ((d >> b) & 1u));
        m &= ((d >> b) & 1u) ? bal : ~bal;
    }
    return m;
}

// Streams read or written once per iteration (optimizer parameters and moments, SH coefficients): the loads and
// stores carry the nontemporal hint (the guide's streaming form: tools/micro/stream measures 6.33 TB/s for
// nontemporal float4 copies against 5.77 TB/s plain); the values are the same bits.  Against plain accesses at
// config-4 mapping: sh_bwd 231 -> 204, map_transform_bwd 90 -> 67, sh_eval 69 -> 36 us.
typedef float gsr_f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float ld_stream(const float* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_stream(float* p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ float4 ld_stream(const float4* p) {
    const gsr_f4v v = __builtin_nontemporal_load(reinterpret_cast<const gsr_f4v*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream(float4* p, float4 v) {
    const gsr_f4v w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<gsr_f4v*>(p));
}

}  // namespace gsr
