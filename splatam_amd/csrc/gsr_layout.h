// gsr_layout.h -- buffer layouts, call parameters and render records of the MI355X-native Gaussian
// rasterizer (gfx950 / CDNA4, wave64).
//
// Buffer layouts are computed on the host from (P, num_rendered, W, H) alone,
// exactly like the reference re-derives its chunk pointers
// (rasterizer_impl.cu:155-194, rasterizer_impl.h:21-73), so gsr_backward can
// find every array again without any header read-back.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace gsr {

constexpr int TILE_X = 16;  // config.h:16-17 (BLOCK_X/BLOCK_Y); parity needs 16x16 tiles
constexpr int TILE_Y = 16;
constexpr int TILE_PIX = TILE_X * TILE_Y;
// Count-matrix rows (one preprocess / duplicate workgroup each): 1024 Gaussians, or 512 when rows of 1024
// would put fewer than two on every CU -- config 3's 293 rows on 256 CUs left 37 CUs with two workgroups'
// work (tracking preprocess 20.3 -> 16.7 us with 586 rows of 512); config 4's 977 rows stay at 1024 (its
// count matrix would double: column scan 16 -> 31 us).  The choice is a pure function of (P, CU count):
// GeomLayout::make and every kernel read it as a shift (Camera::pre_shift).
constexpr int PRE_BLOCK = 1024;  // the largest row (workgroup size bound, LDS arrays)
__host__ __device__ inline int pre_shift_for(int P, int cus) { return ((P + 1023) >> 10) < 2 * cus ? 9 : 10; }
int geom_pre_shift(int P);  // pre_shift_for(P, CU count of the current device) (gsr_capi.hip)
int current_device_cus();   // the current device's CU count (gsr_capi.hip)
constexpr int MAX_LDS_TILES = 16384; // tile histogram in LDS up to 64 KB; global atomics beyond
constexpr int SORT_THREADS = 256;
constexpr int SORT_ITEMS = 8;        // keys per thread per radix pass
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;
constexpr int RADIX = 256;
constexpr int RENDER_BATCH = 256;    // Gaussians staged in LDS per batch
constexpr int INST_REC_MAX = 12;     // backward per-instance record: at most 12 floats (RecLayout)
constexpr int TILE_CTR_STRIDE = 64;  // per-tile atomic counters one 256-B line apart (spread over L2 channels)

// ---------------------------------------------------------------- layouts --
__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// One 64-byte render record per Gaussian (four float4, one cache-line fetch per
// gather in the render kernels; the SoA form cost ~6 line fetches per instance),
// stored in the form the render loops evaluate (copied to LDS as is):
//   q0 = (x, y, K_AC * conic A, K_AC * conic C)   pixel coordinates; K_AC = -log2(e)/2
//   q1 = (K_B * conic B, opacity, depth, workgroup-local instance offset bits); K_B = -log2(e)
//   q2 = (r, g, b, tile rect lo bits)   rect lo = x0 | y0 << 16
//   q3 = (colors2 r, g, b, tile rect hi bits)   rect hi = x1 | y1 << 16; colors2 = 0 unless dual
constexpr int RR_F4 = 4;
struct GeomLayout {       // per-Gaussian state ("geomBuffer")
    size_t rr;            // float4 [P][4] render records
    size_t clamp;         // u32    [P]  SH clamp bits (r, g, b)
    size_t bin;           // uint4  [P]  (rect lo, rect hi, depth bits, tiles) for duplicate
    size_t tiles;         // u32    [P]  tiles touched
    size_t offsets;       // u32    [P]  exclusive instance offset (also in q1.w)
    size_t blocksums;     // u32    [nb] exclusive scan of the per-workgroup instance totals
    size_t wgsum;         // u32    [nb] per-workgroup instance totals (bit 31: prefiltered violation)
    size_t wgcull;        // u32    [nb] per-workgroup culled-instance totals (Camera::cull; point_list's tail)
    size_t counters;      // u32    [8]  [0]=num_rendered [1]=prefiltered violation [2]=longest tile list
                          //             [3]=sort cap [4]=colscan arrival counter
    size_t total;
    int nb;     // count-matrix rows
    int shift;  // log2 Gaussians per row
    static GeomLayout make(int P) { return make(P, geom_pre_shift(P)); }
    static GeomLayout make(int P, int shift) {
        GeomLayout L;
        size_t o = 0, p = (size_t)(P > 0 ? P : 1);
        L.shift = shift;
        L.nb = (P + (1 << shift) - 1) >> shift;
        L.rr = o; o = align_up(o + 16 * RR_F4 * p, 256);
        L.clamp = o; o = align_up(o + 4 * p, 256);
        L.bin = o; o = align_up(o + 16 * p, 256);
        L.tiles = o; o = align_up(o + 4 * p, 256);
        L.offsets = o; o = align_up(o + 4 * p, 256);
        L.blocksums = o; o = align_up(o + 4 * (size_t)(L.nb > 0 ? L.nb : 1), 256);
        L.wgsum = o; o = align_up(o + 4 * (size_t)(L.nb > 0 ? L.nb : 1), 256);
        L.wgcull = o; o = align_up(o + 4 * (size_t)(L.nb > 0 ? L.nb : 1), 256);
        L.counters = o; o = align_up(o + 32, 256);
        L.total = o;
        return L;
    }
};

struct ImgLayout {        // per-pixel / per-tile state ("imgBuffer")
    size_t final_T;       // f32   [N]
    size_t n_contrib;     // u32   [N]
    size_t ranges;        // uint2 [tiles]  [start, end) of each tile's sorted list
    size_t order;         // u32   [tiles]  render schedule: workgroup i renders tile order[i] (tile_plan)
    size_t tile_count;    // u32   [2*tiles*TILE_CTR_STRIDE] instance counters, then bucket cursors (one memset)
    size_t rowmax;        // u32   [tiles*16] per 4x4 block (tile_px/tile_py order): the longest n_contrib
    size_t total;
    static ImgLayout make(int W, int H) {
        ImgLayout L;
        size_t N = (size_t)W * H;
        size_t T = (size_t)((W + TILE_X - 1) / TILE_X) * ((H + TILE_Y - 1) / TILE_Y);
        size_t o = 0;
        L.final_T = o; o = align_up(o + 4 * (N ? N : 1), 256);
        L.n_contrib = o; o = align_up(o + 4 * (N ? N : 1), 256);
        L.ranges = o; o = align_up(o + 8 * (T ? T : 1), 256);
        L.order = o; o = align_up(o + 4 * (T ? T : 1), 256);
        L.tile_count = o; o = align_up(o + 8 * (size_t)TILE_CTR_STRIDE * (T ? T : 1), 256);
        L.rowmax = o; o = align_up(o + 64 * (T ? T : 1), 256);
        L.total = o;
        return L;
    }
};

inline int higher_msb(uint32_t n) {  // rasterizer_impl.cu:35-50 (bits needed for tile ids)
    int b = 0;
    while (b < 32 && (n >> b) != 0) b++;
    return b;
}

constexpr int TILE_SORT_CAP = 4096;  // longest tile list render_fwd sorts (4 chunks of 1024 keys)

struct BinLayout {        // per-instance state ("binningBuffer")
    size_t point_list;    // u64 [I] PointEntry (mask << 32 | Gaussian id) in (tile, depth, id) order -- offset 0
    size_t keys[2];       // u64 [I] bucketed (depth<<32 | id) keys / radix ping-pong (tile<<32 | depth)
    size_t vals[2];       // u32 [I] radix ping-pong values (fallback path only)
    size_t gid;           // u32 [I] Gaussian id of each unsorted instance (fallback path only)
    size_t hist;          // u32 [RADIX * nsb] + [RADIX] digit totals (fallback path only)
    size_t total;
    int nsb;              // radix-sort workgroups
    int npass;            // 8-bit LSD passes over bits [0, 32 + msb(tiles))
    int final_buf;        // which ping-pong half holds the sorted keys/vals
    static BinLayout make(int I, int W, int H) {
        BinLayout L;
        size_t n = (size_t)(I > 0 ? I : 1);
        uint32_t tiles = (uint32_t)(((W + TILE_X - 1) / TILE_X) * ((H + TILE_Y - 1) / TILE_Y));
        int bits = 32 + higher_msb(tiles);
        L.npass = (bits + 7) / 8;
        L.final_buf = L.npass & 1;
        L.nsb = (int)((n + SORT_TILE - 1) / SORT_TILE);
        size_t o = 0;
        L.point_list = o; o = align_up(o + 8 * n, 256);
        L.keys[0] = o; o = align_up(o + 8 * n, 256);
        L.keys[1] = o; o = align_up(o + 8 * n, 256);
        L.vals[0] = o; o = align_up(o + 4 * n, 256);
        L.vals[1] = o; o = align_up(o + 4 * n, 256);
        L.gid = o; o = align_up(o + 4 * n, 256);
        L.hist = o; o = align_up(o + 4 * ((size_t)RADIX * L.nsb + RADIX), 256);  // + digit totals
        L.total = o;
        return L;
    }
};

// ------------------------------------------------------------ parameters --
// A launch's device-side switch (the gated geometry reuse of gsr_forward_reuse_if_equal): the comparison
// kernel stores the call's epoch e into *p when the geometry differs; the kernel runs iff (*p == e) == run.
// The word is not cleared first: whatever it held is not e (epochs are unique per call), which reads as
// "equal" only if the comparison found no difference.  p == nullptr: always runs.  Read once per
// workgroup, before anything else.
struct Gate {
    const uint32_t* p = nullptr;
    uint32_t e = 0;
    uint32_t run = 1;
    __device__ __forceinline__ bool off() const { return p != nullptr && ((*p == e) != (run != 0u)); }
};

struct Camera {
    int W, H;
    float tan_fovx, tan_fovy, focal_x, focal_y;
    int gx, gy;  // tile grid
    const float* view;
    const float* proj;
    const float* campos;
    const float* bg;
    float scale_modifier;
    int sh_degree;
    int prefiltered;
    // Render schedule: render workgroup i renders tile tile_order[i] (a permutation written by
    // the binning's workgroup 0, tile_plan; nullptr = row-major).  sched_cus: the device's CU
    // count, the round size of the plan.
    const uint32_t* tile_order = nullptr;
    uint32_t* tile_order_out = nullptr;
    // Per-block last-contributor maxima (ImgLayout::rowmax): written by render_fwd, read by render_bwd
    // (its batch range and row-list bounds without a reduction over n_contrib first); nullptr = not kept
    uint32_t* rowmax = nullptr;
    int sched_cus = 256;
    int pre_shift = 10;  // log2 Gaussians per count-matrix row (GeomLayout::shift)
    // Tile culling (the fused tracking forward, static mode): a (Gaussian, tile) instance whose alpha >= 1/255
    // ellipse reaches no 4x4 block of the tile (block_mask_exact == 0, conservative) is left out of the tile's
    // bucket -- it would be sorted and staged but never evaluated, and its record would be zero.  Its record
    // slot stays (slots are rect-indexed); bin[i].w carries the Gaussian's live-tile mask, which gauss_bwd
    // reads to skip the unwritten slots.  Results are bitwise those of the unculled lists; num_rendered
    // (the record count) is unchanged, the tile ranges are shorter.
    int cull = 0;
    // point_list's tail [L, num_rendered) of a culled binning: 1 the culled instances themselves (the dynamic
    // forward, whose buffers the caller reads like the reference's), 0 padding ids (static mode)
    int tail_exact = 0;
    Gate gate;  // (preprocess, duplicate_bucket and render_fwd return at once when it is off)
    // Host snapshot (the dynamic forward's bucketed binning only): the duplicate's workgroup 0 stores counters[0..7]
    // into this mapped, coherent pinned host buffer once they are final -- in place of a 32-B device-to-host copy
    // launched behind it (4 us of the stream per forward) -- and the host's event follows the duplicate
    uint32_t* host_snap = nullptr;
};
// bin[i].w: bit k set = rect tile k (row-major in the rect) has an instance in its bucket; all ones when
// nothing is culled (or the rect has more than 32 tiles)
__device__ __forceinline__ bool tile_live(uint32_t live, uint32_t k) { return k >= 32u || ((live >> k) & 1u); }
// culled instances among rect tiles [0, k) (k <= the Gaussian's tile count): positions in point_list's tail
__device__ __forceinline__ uint32_t culled_below(uint32_t live, uint32_t k) {
    const uint32_t m = k >= 32u ? 0xFFFFFFFFu : ((1u << k) - 1u);
    return (uint32_t)__popc(~live & m);
}
// Wave priority by remaining work: the instruction arbiter favours older
// waves, so on a CU the last-dispatched tile used to run alone at the end at one wave per
// SIMD; raising the priority of the waves with the most work left keeps the CU's tiles
// finishing together (a dynamic longest-remaining-first among co-resident tiles).
// Levels at 70 / 45 / 22 % of the frame's mean tile list (`mean4` = 4 x mean, from num_rendered) when every tile
// is resident at once (config 3: 1200 tiles, 1280 workgroup slots; 200 / 100 / 50 % measured 3 us slower
// there), and at 200 / 100 / 50 % when the tiles take several dispatch rounds (config 4: 3225 tiles; the
// single-round levels measured 392 against 383 us for render_bwd): `multi` = more tiles than 5 per CU.
__device__ __forceinline__ void prio_by_remaining(int remaining, uint32_t mean4, bool multi) {
    const uint32_t r = 4u * (uint32_t)remaining;  // compare r / mean4 against the level thresholds (x 100)
    const uint32_t t3 = multi ? 200u : 70u, t2 = multi ? 100u : 45u, t1 = multi ? 50u : 22u;
    if (100u * r > t3 * mean4) __builtin_amdgcn_s_setprio(3);
    else if (100u * r > t2 * mean4) __builtin_amdgcn_s_setprio(2);
    else if (100u * r > t1 * mean4) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}
__device__ __forceinline__ bool sched_multi_round(const Camera& cam) { return cam.gx * cam.gy > 5 * cam.sched_cus; }
__device__ __forceinline__ uint32_t sched_mean4(const Camera& cam, const uint32_t* counters) {
    const uint32_t nt = (uint32_t)(cam.gx * cam.gy);
    return max(1u, (uint32_t)(4ull * counters[0] / (nt ? nt : 1u)));
}
// the tile a render workgroup (1D grid over the tiles) works on
__device__ __forceinline__ int sched_tile(const Camera& cam) {
    return cam.tile_order ? (int)cam.tile_order[blockIdx.x] : (int)blockIdx.x;
}

// SplaTAM's tracking transform (gsr_track_transform_fwd) fused into preprocess: the world-frame
// map + the frame's pose in; preprocess forms the camera-frame rendervars itself and also writes
// them to GaussIn's means3D / rotations / opacities / scales / colors2 (then outputs) for the
// backward.  mw == nullptr: no transform (GaussIn holds the rendervars).
struct TrackXf {
    const float* mw = nullptr;  // means_world [P,3]
    const float* ur = nullptr;  // unnorm_rotations [P,4]
    const float* lo = nullptr;  // logit_opacities [P,1]
    const float* ls = nullptr;  // log_scales [P,scols]
    int scols = 1;
    const float* cq = nullptr;  // the frame's quaternion column (stride qs)
    const float* ct = nullptr;  // the frame's translation column (stride qs)
    int qs = 1;
    const float* w2c = nullptr;  // [16] row-major (depth colours)
    int store = 1;               // 0: the rendervars are not stored (the tracking backward recomputes them)
};

struct GaussIn {
    TrackXf xf;
    int P, M;
    const float* means3D;
    const float* shs;
    const float* colors;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D;
    const float* colors2;  // second precomputed colour set of a dual render (else nullptr)
    int sh_staged;         // SH colours already in bin[i].xyz / clamp (sh_eval_kernel, gsr_sh.hip)
    const uint8_t* alive = nullptr;  // optional per-Gaussian mask, 0 = pruned (gsr_forward_dual_static_alive)
};

struct GeomPtrs {
    float4* rr;
    uint32_t* clamp;
    uint4* bin;
    uint32_t* tiles;
    uint32_t* offsets;
    uint32_t* blocksums;
    uint32_t* counters;
    uint32_t* wgsum;
    uint32_t* wgcull;
    static GeomPtrs at(void* base, const GeomLayout& L) {
        char* b = (char*)base;
        return {(float4*)(b + L.rr), (uint32_t*)(b + L.clamp), (uint4*)(b + L.bin), (uint32_t*)(b + L.tiles),
                (uint32_t*)(b + L.offsets), (uint32_t*)(b + L.blocksums), (uint32_t*)(b + L.counters),
                (uint32_t*)(b + L.wgsum), (uint32_t*)(b + L.wgcull)};
    }
};

// The counter guards a kernel's argument list carries (every file with a render or walk kernel, not only the
// launchers' callers).  Speculative launches: kernels exit early when the device-side counters show
// num_rendered > cap_inst or a tile list longer than cap_tile (the host then
// re-launches with an exact buffer).  Pass UINT32_MAX to disable the guard.
struct SpecGuard {
    const uint32_t* counters;  // GeomLayout counters: [0] num_rendered, [2] longest tile list
    uint32_t cap_inst, cap_tile;
    __device__ __forceinline__ bool overflow() const {
        return counters[0] > cap_inst || counters[2] > cap_tile;
    }
};
// Backward-side check that the forward state is valid for a binning layout of
// `cap_inst` instances: counters[3] holds the longest tile list the sort path
// that produced point_list handles (TILE_SORT_CAP for render_fwd's tile sort,
// 0xffffffff for the radix fallback), set by the forward.  Only a static-mode
// forward can leave it failing; the backward kernels then do no work (no
// out-of-bounds access) and the gradients are zero.
struct BwdGuard {
    const uint32_t* counters;
    uint32_t cap_inst;
    __device__ __forceinline__ bool overflow() const {
        return counters[0] > cap_inst || counters[2] > counters[3];
    }
};
// Static-mode status rows are sticky across calls (HIP-graph replays): [0] and [2] keep the
// maximum num_rendered / longest tile list seen, [1] ORs the prefiltered violations, [3] the
// longest list the tile sort handles.  An overflow in any replay therefore stays visible until
// the caller zeroes the row.
__device__ __forceinline__ void status_merge(uint32_t* st, uint32_t n, uint32_t viol, uint32_t longest,
                                             uint32_t sort_cap) {
    if (n) atomicMax(st + 0, n);
    if (viol) atomicOr(st + 1, viol);
    if (longest) atomicMax(st + 2, longest);
    if (sort_cap) atomicMax(st + 3, sort_cap);
}

// Render record accessors
struct RenderRec {
    float4 q0, q1, q2, q3;
};
__device__ __forceinline__ RenderRec load_rr(const float4* __restrict__ rr, uint32_t i) {
    const float4* r = rr + (size_t)RR_F4 * i;
    return {r[0], r[1], r[2], r[3]};
}
__device__ __forceinline__ uint2 rr_rect(const RenderRec& r) {
    return make_uint2(__float_as_uint(r.q2.w), __float_as_uint(r.q3.w));
}
// instance offset of Gaussian i: scanned workgroup base + workgroup-local part (q1.w)
__device__ __forceinline__ uint32_t rr_offset(const RenderRec& r, const uint32_t* blocksums, uint32_t i, int shift) {
    return blocksums[i >> shift] + __float_as_uint(r.q1.w);
}

// Unsorted instance slot of (Gaussian g, tile tx,ty): duplicateWithKeys order
// (rasterizer_impl.cu:98-109) = offsets[g] + row-major index inside g's tile rect.
__device__ __forceinline__ uint32_t instance_slot(uint2 rect, uint32_t off, uint32_t tx, uint32_t ty) {
    const uint32_t x0 = rect.x & 0xFFFFu, y0 = rect.x >> 16, w = (rect.y & 0xFFFFu) - x0;
    return off + (ty - y0) * w + (tx - x0);
}

}  // namespace gsr
