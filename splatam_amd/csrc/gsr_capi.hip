// gsr_capi.hip -- extern "C" entry points of libgsr.so (see include/gsr.h).
//
// Host orchestration of one rasterization, the counterpart of
// CudaRasterizer::Rasterizer::{forward,backward,markVisible}
// (rasterizer_impl.cu:141-434).  Everything is enqueued on the caller's
// stream; the only host synchronisation is the read-back of num_rendered
// (the reference's cudaMemcpy at rasterizer_impl.cu:282), done through a
// pinned per-thread staging word.
//
// Every entry point fills a call record (FwdCall / BwdCall) by name; the forward runs as the steps of
// `Forward`, the backward as one function per gradient path over `Backward`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <string>

#include "../../include/gsr.h"
#include "../../include/gsr_glue.h"
#include "gsr_adam.h"
#include "gsr_errors.h"
#include "gsr_host.h"
#include "gsr_launch.h"
#include "gsr_layout.h"

using namespace gsr;

namespace {
thread_local std::string g_last_error;

// resets as kernels: plain kernel nodes when captured in a HIP graph (small memcpy /
// memset nodes misbehaved on re-replay here)
__global__ void zero_words_kernel(uint32_t* __restrict__ p, size_t n) {
    for (size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) p[k] = 0u;
}
std::atomic<int> g_cus[kMaxDevices];  // CU count per device (render schedule round size), 0 = unknown
}  // namespace

namespace gsr {
int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char* where) {
    return fail(GSR_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

int check_terms(const char* entry, const float* terms) {
    if (!terms) return fail(GSR_ERR_INVALID_ARG, std::string(entry) + ": null terms");
    if ((uintptr_t)terms % sizeof(float) != 0)
        return fail(GSR_ERR_INVALID_ARG, std::string(entry) + ": terms must be 4-byte aligned");
    return GSR_OK;
}

int stream_device(hipStream_t s) {
    thread_local hipStream_t last_s = nullptr;
    thread_local int last_d = -1;
    if (last_d >= 0 && s == last_s && s != nullptr) return last_d;
    int d = 0;
    if (hipStreamGetDevice(s, &d) != hipSuccess && hipGetDevice(&d) != hipSuccess) d = 0;
    (void)hipGetLastError();
    if (d < 0 || d >= kMaxDevices) d = 0;
    last_s = s;
    last_d = d;
    return d;
}
int current_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) d = 0;
    return d;
}
int device_cus(int dev) {
    int n = g_cus[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    (void)hipGetLastError();
    g_cus[dev].store(n, std::memory_order_relaxed);
    return n;
}
hipError_t zero_async(void* p, size_t bytes, hipStream_t s) {
    const size_t n = bytes / 4;
    if (n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>(1024, (n + 255) / 256);
    hipLaunchKernelGGL(zero_words_kernel, dim3(blocks), dim3(256), 0, s, (uint32_t*)p, n);
    return hipGetLastError();
}
int geom_pre_shift(int P) { return pre_shift_for(P, device_cus(current_device())); }
int current_device_cus() { return device_cus(current_device()); }
}  // namespace gsr

namespace {

struct Pinned {  // per-thread staging of the device counters + the event after the scan
    uint32_t* p = nullptr;   // (mapped, coherent: the bucketed duplicate stores into it, Camera::host_snap)
    uint32_t* dp = nullptr;  // its device address
    hipEvent_t ev = nullptr;
    ~Pinned() {
        if (p) (void)hipHostFree(p);
        if (ev) (void)hipEventDestroy(ev);
    }
    int ensure(int dev) {
        hipError_t e;
        if (!p) {
            // (portable: the buffer serves the launches on device `dev`, whatever device is current here)
            if ((e = hipHostMalloc((void**)&p, 32,
                                   hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable)) != hipSuccess)
                return hip_fail(e, "hipHostMalloc");
            if ((e = hipHostGetDevicePointer((void**)&dp, p, 0)) != hipSuccess)
                return hip_fail(e, "hipHostGetDevicePointer");
        }
        if (!ev) {  // created on the stream's device (the caller's current device is that device)
            int cur = 0;
            (void)hipGetDevice(&cur);
            if (cur != dev) (void)hipSetDevice(dev);
            e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            if (cur != dev) (void)hipSetDevice(cur);
            if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
        }
        return GSR_OK;
    }
};
thread_local Pinned g_pinned[kMaxDevices];
// GSR_SNAP_COPY=1: the counters reach the host by a copy launched after the duplicate (A/B switch of Camera::host_snap)
const bool g_snap_copy = getenv("GSR_SNAP_COPY") && atoi(getenv("GSR_SNAP_COPY")) != 0;
struct RatioHint {
    std::atomic<double> v{3.0};  // last num_rendered / P (binning capacity hint)
};
RatioHint g_inst_ratio[kMaxDevices];

Camera make_camera(const gsr_settings* s) {
    Camera c;
    c.W = s->image_width;
    c.H = s->image_height;
    c.tan_fovx = s->tan_fovx;
    c.tan_fovy = s->tan_fovy;
    c.focal_y = (float)c.H / (2.0f * s->tan_fovy);  // rasterizer_impl.cu:222-223
    c.focal_x = (float)c.W / (2.0f * s->tan_fovx);
    c.gx = (c.W + TILE_X - 1) / TILE_X;
    c.gy = (c.H + TILE_Y - 1) / TILE_Y;
    c.view = s->viewmatrix;
    c.proj = s->projmatrix;
    c.campos = s->campos;
    c.bg = s->bg;
    c.scale_modifier = s->scale_modifier;
    c.sh_degree = s->sh_degree;
    c.prefiltered = s->prefiltered;
    return c;
}

GaussIn make_gauss(const gsr_gaussians* g) {
    GaussIn o;
    o.P = g->P;
    o.M = g->shs ? g->M : 0;
    o.means3D = g->means3D;
    o.shs = (g->shs && g->M > 0) ? g->shs : nullptr;
    o.colors = g->colors_precomp;
    o.opacities = g->opacities;
    o.scales = g->scales;
    o.rotations = g->rotations;
    o.cov3D = g->cov3D_precomp;
    o.colors2 = nullptr;
    o.sh_staged = 0;
    o.alive = nullptr;
    return o;
}

int validate(const gsr_settings* s, const gsr_gaussians* g, bool forward) {
    if (!s || !g) return fail(GSR_ERR_INVALID_ARG, "null settings or gaussians");
    if (g->P < 0) return fail(GSR_ERR_INVALID_ARG, "P must be >= 0");
    if (s->binning != GSR_BINNING_CULLED && s->binning != GSR_BINNING_REFERENCE)
        return fail(GSR_ERR_INVALID_ARG, "settings.binning must be GSR_BINNING_CULLED or GSR_BINNING_REFERENCE");
    if (s->image_width <= 0 || s->image_height <= 0) return fail(GSR_ERR_INVALID_ARG, "image size must be positive");
    if (s->image_width > 16 * 65535 || s->image_height > 16 * 65535)
        return fail(GSR_ERR_INVALID_ARG, "image too large for 16-bit tile coordinates");
    if (g->P == 0) return GSR_OK;
    if (!g->means3D) return fail(GSR_ERR_INVALID_ARG, "means3D is required");
    if (forward && !g->opacities) return fail(GSR_ERR_INVALID_ARG, "opacities are required");
    if (!s->viewmatrix || !s->projmatrix || !s->bg) return fail(GSR_ERR_INVALID_ARG, "camera matrices / bg missing");
    const bool has_sh = g->shs && g->M > 0;
    if (!g->colors_precomp && !has_sh)
        return fail(GSR_ERR_INVALID_ARG, "Please provide excatly one of either SHs or precomputed colors!");
    if (!g->colors_precomp && !s->campos) return fail(GSR_ERR_INVALID_ARG, "campos required for SH colours");
    if (has_sh && (s->sh_degree < 0 || s->sh_degree > 3 || (s->sh_degree + 1) * (s->sh_degree + 1) > g->M))
        return fail(GSR_ERR_INVALID_ARG, "sh_degree must be in [0,3] with (deg+1)^2 <= M");
    const bool has_sr = g->scales && g->rotations;
    if (!has_sr && !g->cov3D_precomp)
        return fail(GSR_ERR_INVALID_ARG,
                    "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    return GSR_OK;
}

// one buffer from the caller's allocator; NULL is GSR_ERR_ALLOC "allocator returned NULL (<what>)"
template <class T>
int obtain(gsr_alloc_fn alloc, void* ctx, int kind, size_t bytes, const char* what, T** out) {
    *out = (T*)alloc(ctx, kind, bytes);
    return *out ? GSR_OK : fail(GSR_ERR_ALLOC, std::string("allocator returned NULL (") + what + ")");
}

// gsr_forward_reuse_if_equal's inputs: the device comparison and the previous call's state
struct ReuseIn {
    EqualPairs pairs;
    int prev_num_rendered;
    const void* prev_geom;
    void* prev_binning;
    void* prev_image;
    const int* prev_radii;
    int* reused;
};

// One forward call.  colors2 != NULL: dual render (second colour set composited in the same pass, out_color2).
// capacity > 0: static mode -- binning buffer of `capacity` instances, no host synchronisation at all
// (graph-capturable); the device counters are copied to `status` and the call returns `capacity` (the layout
// size for the backward).  l1: the tracking L1 loss in the render's epilogue; xf: the tracking transform fused
// into preprocess; track_inst: the fused tracking render backward's records; reuse: the gated geometry reuse.
struct FwdCall {
    const gsr_settings* settings = nullptr;
    const gsr_gaussians* gaussians = nullptr;
    const float* colors2 = nullptr;
    float* out_color = nullptr;
    float* out_color2 = nullptr;
    float* out_depth = nullptr;
    int* radii = nullptr;
    gsr_alloc_fn alloc = nullptr;
    void* alloc_ctx = nullptr;
    void* stream = nullptr;
    int capacity = 0;
    uint32_t* status = nullptr;
    const TrackL1* l1 = nullptr;
    const TrackXf* xf = nullptr;
    float* track_inst = nullptr;
    const uint8_t* alive = nullptr;
    const ReuseIn* reuse = nullptr;
};

// the group every forward entry passes: inputs, the first image and depth, radii, allocator, stream
FwdCall fwd_call(const gsr_settings* settings, const gsr_gaussians* gaussians, float* out_color, float* out_depth,
                 int* radii, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    FwdCall c;
    c.settings = settings; c.gaussians = gaussians;
    c.out_color = out_color; c.out_depth = out_depth; c.radii = radii;
    c.alloc = alloc; c.alloc_ctx = alloc_ctx; c.stream = stream;
    return c;
}
FwdCall& dual(FwdCall& c, const float* colors2, float* out_color2) {  // the second colour set and its image
    c.colors2 = colors2; c.out_color2 = out_color2;
    return c;
}
FwdCall& statics(FwdCall& c, int capacity, uint32_t* status) {
    c.capacity = capacity; c.status = status;
    return c;
}

// the fused tracking render may leave its images unstored (all three image pointers NULL): its loss and
// backward consume them in registers
bool stores_no_images(const FwdCall& c) { return c.track_inst && !c.out_color && !c.out_color2 && !c.out_depth; }

int check_forward(const FwdCall& c) {
    const int rc = validate(c.settings, c.gaussians, true);
    if (c.track_inst && (!c.l1 || !c.colors2 || c.capacity <= 0))
        return fail(GSR_ERR_INVALID_ARG, "the fused render backward needs the static dual forward with the L1 loss");
    if (rc != GSR_OK) return rc;
    if (!c.alloc) return fail(GSR_ERR_INVALID_ARG, "allocator callback required");
    if (!stores_no_images(c)) {
        if (!c.out_color || !c.out_depth) return fail(GSR_ERR_INVALID_ARG, "output image pointers required");
        if (c.colors2 && !c.out_color2) return fail(GSR_ERR_INVALID_ARG, "out_color2 required with colors2");
    }
    if (c.colors2 && c.gaussians->P > 0 && !c.gaussians->means3D)
        return fail(GSR_ERR_INVALID_ARG, "means3D is required");
    return GSR_OK;
}

// The forward's state and its steps, in launch order (forward_impl below).
struct Forward {
    const FwdCall& c;
    hipStream_t stream;
    int dev;
    Pinned& pin;
    Camera cam;
    GaussIn g;
    int P, W, H, ntiles;
    GeomLayout GL;
    ImgLayout IL;
    void* geom = nullptr;
    GeomPtrs geo{};
    ImgPtrs img{};
    uint32_t* cursor = nullptr;
    // tile counts: per-workgroup LDS histograms + column scan (transient count matrix in SCRATCH),
    // or global atomics on padded counters when the histogram does not fit in LDS
    bool lds_hist;
    uint32_t* cmat = nullptr;
    uint32_t* tile_tot = nullptr;
    bool force_radix;
    // the bucketed duplicate does the instance / tile scans itself (lds_hist); otherwise a
    // scan launch does them, and the counters are final right after it
    bool scan_in_duplicate;
    bool eager;  // capacity <= 0: the host reads the counters
    bool gated = false;
    Gate eq_gate;
    uint32_t epoch = 0;
    uint32_t cap = 0;  // instances the speculative binning buffer holds

    static bool force_radix_env() {  // GSR_FORCE_RADIX, read at the first forward
        static const bool on = getenv("GSR_FORCE_RADIX") && atoi(getenv("GSR_FORCE_RADIX")) != 0;
        return on;
    }
    explicit Forward(const FwdCall& call)
        : c(call), stream((hipStream_t)call.stream), dev(stream_device(stream)), pin(g_pinned[dev]),
          cam(make_camera(call.settings)), g(make_gauss(call.gaussians)), P(g.P), W(cam.W), H(cam.H),
          ntiles(cam.gx * cam.gy), GL(GeomLayout::make(P)), IL(ImgLayout::make(W, H)),
          lds_hist(ntiles <= MAX_LDS_TILES), force_radix(force_radix_env() && call.capacity <= 0),
          scan_in_duplicate(lds_hist && !force_radix), eager(call.capacity <= 0) {
        g.colors2 = c.colors2;  // packed into the render records by preprocess (dual render)
        g.alive = c.alive;
        if (c.xf) g.xf = *c.xf;  // tracking transform fused into preprocess (g's arrays are then its outputs)
        cam.pre_shift = GL.shift;
        // tile culling: a per-call choice (gsr_settings.binning), no process-wide mode
        cam.cull = c.settings->binning != GSR_BINNING_REFERENCE ? 1 : 0;
        cam.tail_exact = eager ? 1 : 0;  // (include/gsr.h: the culled instances, or padding in static mode)
    }
    uint32_t* status() const { return eager ? nullptr : c.status; }
    template <class T>
    int obtain(int kind, size_t bytes, const char* what, T** out) {
        return ::obtain(c.alloc, c.alloc_ctx, kind, bytes, what, out);
    }

    int setup_buffers() {
        void* image = nullptr;
        geom = c.alloc(c.alloc_ctx, GSR_BUF_GEOM, GL.total);
        image = c.alloc(c.alloc_ctx, GSR_BUF_IMAGE, IL.total);
        if (!geom || !image) return fail(GSR_ERR_ALLOC, "allocator returned NULL (geom/image buffer)");
        geo = GeomPtrs::at(geom, GL);
        img = ImgPtrs::at(image, IL);
        bind_schedule(cam, img, dev);
        cursor = img.tile_count + (size_t)ntiles * TILE_CTR_STRIDE;
        hipError_t e;
        if (lds_hist && P > 0) {
            if (int rc = obtain(GSR_BUF_SCRATCH, 4 * ((size_t)GL.nb * ntiles + ntiles), "tile count matrix", &cmat))
                return rc;
            tile_tot = cmat + (size_t)GL.nb * ntiles;
        } else if ((e = zero_async(img.tile_count, 8 * (size_t)ntiles * TILE_CTR_STRIDE, stream)) != hipSuccess) {
            return hip_fail(e, "memset tile counts");
        }
        if (c.reuse && c.reuse->reused) *c.reuse->reused = 0;
        return GSR_OK;
    }

    // rasterize_points.cu:67-81: zero outputs, forward not run (the sticky status keeps its rows)
    int empty_map() {
        hipError_t e;
        if ((e = zero_async(img.ranges, sizeof(uint2) * (size_t)ntiles, stream)) != hipSuccess)
            return hip_fail(e, "memset ranges");
        void* bin;
        if (int rc = obtain(GSR_BUF_BINNING, BinLayout::make(0, W, H).total, "binning buffer", &bin)) return rc;
        const size_t img3 = sizeof(float) * 3 * (size_t)W * H;
        if (const TrackL1* l1 = c.l1) {  // the zero silhouette masks every pixel: loss 0 and zero gradient images
            if ((e = zero_async(l1->loss, sizeof(float), stream)) != hipSuccess ||
                (l1->terms && (e = zero_async(l1->terms, 2 * sizeof(float), stream)) != hipSuccess) ||
                (l1->dL_dim && (e = zero_async(l1->dL_dim, img3, stream)) != hipSuccess) ||
                (l1->dL_dds && (e = zero_async(l1->dL_dds, img3, stream)) != hipSuccess))
                return hip_fail(e, "zero loss");
        }
        if (stores_no_images(c)) return 0;
        if ((e = zero_async(c.out_color, img3, stream)) != hipSuccess ||
            (e = zero_async(c.out_depth, sizeof(float) * (size_t)W * H, stream)) != hipSuccess ||
            (c.colors2 && (e = zero_async(c.out_color2, img3, stream)) != hipSuccess))
            return hip_fail(e, "zero outputs");
        return 0;
    }

    // gated geometry reuse (gsr_forward_reuse_if_equal): the device compares this call's geometry with the
    // previous call's, both forms are enqueued with every launch gated on the result (counters[5]), and the
    // host learns which one ran from the counter copy it waits on anyway -- no second synchronisation.  (A
    // speculative form -- the reuse enqueued unconditionally, the host waiting on the comparison right after
    // it, the full forward only on a difference -- measured slower on the unchanged caller: its early wait
    // stalls the host before the call's render is enqueued, profiles/r10i_unit_reuse_forms.txt)
    int gate_on_comparison() {
        gated = c.reuse && eager && !c.colors2 && !c.track_inst && !c.l1 && !c.xf && lds_hist && !force_radix &&
                !sh_staged(cam, g);
        if (!gated) return GSR_OK;
        // the comparison word is counters[5] of this call's geometry buffer, not cleared: the comparison stores
        // this call's epoch there on a difference.  Epochs are unique per call, but the buffer is recycled
        // memory, so the word may by chance already hold this epoch; the call then reads as "different" and
        // runs the full forward although the geometry is equal -- the slower form, with the same results.
        // Nothing can make a differing geometry read as equal.
        static std::atomic<uint32_t> g_epoch{0};
        do epoch = g_epoch.fetch_add(1u, std::memory_order_relaxed) + 1u; while (epoch == 0u);
        uint32_t* word = geo.counters + 5;
        hipError_t e;
        if ((e = launch_epoch_mismatch(c.reuse->pairs, word, epoch, stream)) != hipSuccess)
            return hip_fail(e, "geometry comparison");
        cam.gate = Gate{word, epoch, 1u};  // the full forward runs when the geometry differs ...
        eq_gate = Gate{word, epoch, 0u};   // ... the reuse form when it is equal
        if ((e = launch_reuse_copy(eq_gate, c.reuse->prev_geom, geom, GL.counters, GL.tiles, g.colors,
                                   c.reuse->prev_radii, c.radii, P, stream)) != hipSuccess)
            return hip_fail(e, "geometry reuse");
        return GSR_OK;
    }

    // num_rendered & co. to pinned host memory (eager mode): copied here, or (stored_by_kernel) already stored by
    // the launch just enqueued (Camera::host_snap)
    int snapshot_counters(bool stored_by_kernel) {
        if (int rc = pin.ensure(dev)) return rc;
        hipError_t e;
        if (!stored_by_kernel &&
            (e = hipMemcpyAsync(pin.p, geo.counters, 32, hipMemcpyDeviceToHost, stream)) != hipSuccess)
            return hip_fail(e, "copy num_rendered");
        if ((e = hipEventRecord(pin.ev, stream)) != hipSuccess) return hip_fail(e, "record num_rendered");
        return GSR_OK;
    }

    int counts_and_ranges() {
        hipError_t e;
        // the bucketed duplicate's workgroup 0 writes the render schedule (tile_plan); the other paths
        // render in row-major order
        if (!scan_in_duplicate && (e = launch_identity_order(img.order, ntiles, stream)) != hipSuccess)
            return hip_fail(e, "render schedule");
        if (!c.radii) return fail(GSR_ERR_INVALID_ARG, "radii output required");
        {
            // (stage clocks in the device-clock mode: preprocess_kernel stamps itself; sh_eval is not timed)
            StageTimer t(GSR_STAGE_PREPROCESS, P, stream, true);
            if (sh_staged(cam, g)) {  // SH colours with coalesced coefficient reads, ahead of preprocess
                if ((e = launch_sh_eval(cam, g, geo, stream)) != hipSuccess) return hip_fail(e, "sh_eval");
                g.sh_staged = 1;
            }
            if ((e = launch_preprocess(cam, g, geo, c.radii, lds_hist ? cmat : img.tile_count, lds_hist, ntiles,
                                       GL.nb, stream, t.kclock())) != hipSuccess)
                return hip_fail(e, "preprocess");
        }
        {
            // the tile-count scans that give the ranges (the "ranges" stage of the bucketed path)
            StageTimer t(GSR_STAGE_RANGES, ntiles, stream, lds_hist);
            if (lds_hist) {  // column scan (+ instance / tile scans in the same launch unless scan_in_duplicate)
                if ((e = launch_tile_colscan(cmat, GL.nb, ntiles, tile_tot, geo, img.ranges, status(),
                                             !scan_in_duplicate, stream, t.kclock(), cam.gate)) != hipSuccess)
                    return hip_fail(e, "tile count scan");
            } else if ((e = launch_scan_counts(geo, GL.nb, img.tile_count, TILE_CTR_STRIDE, ntiles, img.ranges,
                                               status(), stream)) != hipSuccess) {
                return hip_fail(e, "scan");
            }
        }
        if (eager && !scan_in_duplicate) return snapshot_counters(false);
        return GSR_OK;
    }

    // units: the stage's work (0 for a speculative launch, which learns it after the host wait)
    int render(const BinPtrs& bin, uint64_t* keys, const SpecGuard& guard, long long units) {
        StageTimer t(GSR_STAGE_RENDER_FWD, units, stream, true);
        hipError_t e;
        if (c.track_inst) {  // forward + L1 + the tracking render backward, one launch (render_track_kernel)
            if ((e = launch_render_track(cam, img.ranges, bin.point_list, keys, geo,
                                         stores_no_images(c) ? nullptr : img.final_T, img.n_contrib, c.out_color,
                                         c.out_color2, c.out_depth, guard, *c.l1, c.track_inst, stream,
                                         t.kclock())) != hipSuccess)
                return hip_fail(e, "render (fused tracking forward + backward)");
        } else if ((e = launch_render_fwd(cam, img.ranges, bin.point_list, keys, geo, c.colors2, img.final_T,
                                          img.n_contrib, c.out_color, c.out_color2, c.out_depth, guard, stream,
                                          t.kclock(), c.l1)) != hipSuccess) {
            return hip_fail(e, "render");
        }
        return GSR_OK;
    }

    // the bucketed duplicate (its per-tile sort is render_fwd's prologue) and the render.  host_snap: the
    // duplicate stores the counters to pinned memory itself; snapshot: the host will wait for them
    int duplicate_render(const BinPtrs& bin, const SpecGuard& guard, uint32_t* host_snap, bool snapshot,
                         long long units) {
        Camera cplan = cam;
        cplan.tile_order_out = scan_in_duplicate ? img.order : nullptr;
        cplan.host_snap = host_snap;
        {
            StageTimer t(GSR_STAGE_DUPLICATE, P, stream, true);
            hipError_t e = launch_duplicate_bucket(cplan, P, geo, img.ranges, tile_tot, lds_hist ? cmat : cursor,
                                                   lds_hist, ntiles, bin.keys[0], bin.point_list, GL.nb, guard,
                                                   status(), stream, t.kclock());
            if (e != hipSuccess) return hip_fail(e, "duplicate");
        }
        if (snapshot)
            if (int rc = snapshot_counters(host_snap != nullptr)) return rc;
        return render(bin, bin.keys[0], guard, units);
    }

    // Speculative binning + render: the binning buffer is sized from the last
    // calls' instances-per-Gaussian ratio, so everything is enqueued before the
    // host waits on num_rendered (the reference blocks right after the scan,
    // rasterizer_impl.cu:282, leaving the GPU idle while it launches the rest).
    int speculate() {
        void* buf;
        if (int rc = obtain(GSR_BUF_BINNING, BinLayout::make((int)cap, W, H).total, "binning buffer", &buf)) return rc;
        const BinPtrs bin = BinPtrs::at(buf, BinLayout::make((int)cap, W, H));
        const bool snapshot = eager && scan_in_duplicate;
        const bool dup_snap = snapshot && !g_snap_copy;
        if (dup_snap)
            if (int rc = pin.ensure(dev)) return rc;
        const SpecGuard guard{geo.counters, cap, (uint32_t)TILE_SORT_CAP};
        if (int rc = duplicate_render(bin, guard, dup_snap ? pin.dp : nullptr, snapshot, 0)) return rc;
        if (gated) {  // the reuse form's render: the previous call's sorted lists (no sort), ranges, schedule
                      // and image buffer (its final_T / n_contrib rewritten with the same values), this call's
                      // records (the copied geometry)
            Camera cr = cam;
            cr.gate = eq_gate;
            const ImgPtrs prev = ImgPtrs::at(c.reuse->prev_image, IL);
            bind_schedule(cr, prev, dev);
            const SpecGuard rg{geo.counters, (uint32_t)c.reuse->prev_num_rendered, 0xFFFFFFFFu};
            hipError_t e = launch_render_fwd(cr, prev.ranges, (uint64_t*)c.reuse->prev_binning, nullptr, geo, nullptr,
                                             prev.final_T, prev.n_contrib, c.out_color, nullptr, c.out_depth, rg,
                                             stream);
            if (e != hipSuccess) return hip_fail(e, "render (geometry reuse)");
        }
        return GSR_OK;
    }

    // fallback for tiles longer than the LDS sort: global stable LSD radix sort of (tile, depth)
    int radix_binning(const BinPtrs& bin, const BinLayout& BL, uint32_t I) {
        hipError_t e;
        if ((e = hipMemsetD32Async((hipDeviceptr_t)(geo.counters + 3), 0xffffffffu, 1, stream)) != hipSuccess)
            return hip_fail(e, "sort path flag");
        {
            StageTimer t(GSR_STAGE_DUPLICATE, P, stream);
            if ((e = launch_duplicate(cam, P, geo, bin.keys[0], bin.gid, GL.nb, stream)) != hipSuccess)
                return hip_fail(e, "duplicate");
        }
        {
            StageTimer t(GSR_STAGE_SORT, I, stream);
            uint64_t* keys[2] = {bin.keys[0], bin.keys[1]};
            uint32_t* vals[2] = {bin.vals[0], bin.vals[1]};
            if ((e = launch_radix_sort(keys, vals, bin.hist, I, BL.nsb, BL.npass, stream)) != hipSuccess)
                return hip_fail(e, "radix sort");
        }
        StageTimer t(GSR_STAGE_RANGES, I, stream);
        if ((e = launch_gather_ids(bin.vals[BL.final_buf], bin.gid, bin.point_list, I, stream)) != hipSuccess)
            return hip_fail(e, "gather ids");
        return GSR_OK;
    }

    // the host waits for the counters and decides: the reuse form ran, the speculative launches hold, or an
    // exact re-launch (capacity overflow, a tile longer than the LDS sort, or forced radix)
    int wait_and_finish() {
        hipError_t e;
        if ((e = hipEventSynchronize(pin.ev)) != hipSuccess) return hip_fail(e, "sync num_rendered");
        if (gated && pin.p[5] != epoch) {  // equal geometry: the reuse form ran (num_rendered is the previous call's)
            *c.reuse->reused = 1;
            return c.reuse->prev_num_rendered;
        }
        const uint32_t I = pin.p[0];
        const uint32_t longest = pin.p[2];
        if (pin.p[1] != 0)
            return fail(GSR_ERR_PREFILTERED, "Point is filtered although prefiltered is set. This shouldn't happen!");
        if (I > 0x7fffffffu) return fail(GSR_ERR_INVALID_ARG, "num_rendered overflows int32");
        g_inst_ratio[dev].v.store(std::max(0.05, (double)I / P), std::memory_order_relaxed);
        if (!force_radix && I <= cap && longest <= (uint32_t)TILE_SORT_CAP) {
            g_timing_units(dev, GSR_STAGE_SORT, I);
            g_timing_units(dev, GSR_STAGE_RENDER_FWD, I);
            return (int)I;
        }
        const BinLayout BL = BinLayout::make((int)I, W, H);
        void* buf;
        if (int rc = obtain(GSR_BUF_BINNING, BL.total, "binning buffer", &buf)) return rc;
        const BinPtrs bin = BinPtrs::at(buf, BL);
        const SpecGuard none{geo.counters, 0xffffffffu, 0xffffffffu};
        int rc;
        if (I > 0 && longest <= (uint32_t)TILE_SORT_CAP && !force_radix) {
            // (host_snap NULL: the host has read this call's counters, nothing may store into them later)
            rc = duplicate_render(bin, none, nullptr, false, I);
        } else {
            rc = I > 0 ? radix_binning(bin, BL, I) : GSR_OK;
            if (rc == GSR_OK) rc = render(bin, nullptr, none, I);
        }
        return rc != GSR_OK ? rc : (int)I;
    }
};

int forward_impl(const FwdCall& c) {
    if (int rc = check_forward(c)) return rc;
    Forward F(c);
    if (int rc = F.setup_buffers()) return rc;
    if (F.P == 0) return F.empty_map();
    int rc;
    if ((rc = F.gate_on_comparison()) != GSR_OK || (rc = F.counts_and_ranges()) != GSR_OK) return rc;
    const double ratio = g_inst_ratio[F.dev].v.load(std::memory_order_relaxed);
    F.cap = F.eager ? (uint32_t)std::min(2.0e9, std::max(1024.0, 1.5 * ratio * F.P)) : (uint32_t)c.capacity;
    if (!F.force_radix && (rc = F.speculate()) != GSR_OK) return rc;
    if (!F.eager) return (int)F.cap;  // static mode: report, never wait (an overflow shows in status, outputs invalid)
    return F.wait_and_finish();
}

// One backward call: the forward's inputs and state, the incoming gradients and the requested outputs.
// pose: the pose-fused tracking backward; sh_adam: the colour group's Adam step inside the SH backward;
// pre_inst: records already formed by the fused tracking render (the gradient images are then not read).
struct BwdCall {
    const gsr_settings* settings = nullptr;
    const gsr_gaussians* gaussians = nullptr;
    const int* radii = nullptr;
    const float* dL_dout_color = nullptr;
    const float* colors2 = nullptr;
    const float* dL_dout_color2 = nullptr;
    int num_rendered = 0;
    const void* geom_buffer = nullptr;
    const void* binning_buffer = nullptr;
    const void* image_buffer = nullptr;
    int power = 1;
    const gsr_grads* grads = nullptr;
    float* dcolors2 = nullptr;
    int dl2_channels = 3;
    gsr_alloc_fn alloc = nullptr;
    void* alloc_ctx = nullptr;
    void* stream = nullptr;
    const PoseFuse* pose = nullptr;
    const ShAdam* sh_adam = nullptr;
    const float* pre_inst = nullptr;
    float* dmeans2D_c1 = nullptr;  // gsr_backward_dual_m2d: the first colour set's own means2D gradient
};

// the group every backward entry passes: inputs, radii and the forward's state ...
BwdCall bwd_call(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii, int num_rendered,
                 const void* geom_buffer, const void* binning_buffer, const void* image_buffer) {
    BwdCall c;
    c.settings = settings; c.gaussians = gaussians; c.radii = radii; c.num_rendered = num_rendered;
    c.geom_buffer = geom_buffer; c.binning_buffer = binning_buffer; c.image_buffer = image_buffer;
    return c;
}
BwdCall& on(BwdCall& c, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {  // ... and allocator, stream
    c.alloc = alloc; c.alloc_ctx = alloc_ctx; c.stream = stream;
    return c;
}

// The backward's state and one function per gradient path (backward_impl below chooses).
struct Backward {
    const BwdCall& c;
    hipStream_t stream;
    Camera cam;
    GaussIn g;
    int P, R;  // R: num_rendered
    GeomPtrs geo{};
    ImgPtrs img{};
    const uint64_t* point_list = nullptr;
    GradsOut out;
    BwdGuard guard{};

    explicit Backward(const BwdCall& call)
        : c(call), stream((hipStream_t)call.stream), cam(make_camera(call.settings)),
          g(make_gauss(call.gaussians)), P(g.P), R(call.num_rendered),
          out{c.grads->dmeans2D, c.grads->dcolors, c.grads->dopacity, c.grads->dmeans3D,
              c.grads->dcov3D,   c.grads->dsh,     c.grads->dscales,  c.grads->drotations} {}

    void bind_forward_state() {
        const GeomLayout GL = GeomLayout::make(P);
        cam.pre_shift = GL.shift;
        geo = GeomPtrs::at(const_cast<void*>(c.geom_buffer), GL);
        img = ImgPtrs::at(const_cast<void*>(c.image_buffer), ImgLayout::make(cam.W, cam.H));
        bind_schedule(cam, img, current_device());
        if (c.binning_buffer)
            point_list = (const uint64_t*)((const char*)c.binning_buffer + BinLayout::make(R, cam.W, cam.H).point_list);
        guard = BwdGuard{geo.counters, (uint32_t)R};
    }

    // the checks the backward_power != 1 paths share, then their scratch (none for bytes == 0)
    int power_scratch(size_t bytes, char** scratch) {
        *scratch = nullptr;
        if (R > 0 && !c.binning_buffer) return fail(GSR_ERR_INVALID_ARG, "missing binning buffer");
        if (!c.alloc) return fail(GSR_ERR_INVALID_ARG, "allocator callback required");
        if (bytes == 0) return GSR_OK;
        return obtain(c.alloc, c.alloc_ctx, GSR_BUF_SCRATCH, bytes, "backward scratch", scratch);
    }

    // Fisher-selective path: only dL/dmeans3D (+ dL/dopacity), the gradients the fork's Fisher
    // scoring reads (scripts/ros_handler.py:884-889)
    int fisher() {
        if (g.shs) return fail(GSR_ERR_INVALID_ARG, "backward_power != 1 with only dmeans3D / dopacity requested "
                                                    "needs precomputed colours (no SH)");
        const size_t mp_bytes = align_up(sizeof(float) * MPACK_FLOATS * (size_t)P, 256);
        char* scratch;
        if (int rc = power_scratch(mp_bytes + sizeof(float) * 4 * (size_t)R, &scratch)) return rc;
        float* mpack = (float*)scratch;
        float* rec = (float*)(scratch + mp_bytes);
        hipError_t e;
        {
            StageTimer t(GSR_STAGE_GAUSS_BWD, P, stream);
            if ((e = launch_gauss_mpack(cam, g, c.radii, mpack, stream)) != hipSuccess)
                return hip_fail(e, "gaussian chain matrix");
        }
        if (R > 0) {
            StageTimer t(GSR_STAGE_RENDER_BWD, R, stream);
            if ((e = launch_render_bwd_fisher(cam, img.ranges, point_list, geo, mpack, img.final_T, img.n_contrib,
                                              c.dL_dout_color, c.power, rec, guard, stream)) != hipSuccess)
                return hip_fail(e, "render backward (fisher)");
        }
        StageTimer t(GSR_STAGE_GAUSS_BWD, P, stream);
        if ((e = launch_gauss_bwd_fisher(P, geo, c.radii, rec, out.dmeans3D, out.dopacity, guard, stream)) !=
            hipSuccess)
            return hip_fail(e, "gaussian backward (fisher)");
        return GSR_OK;
    }

    // backward_power == 2 (the fork's Fisher / Hessian scoring, scripts/ros_handler.py:839-902): each
    // pair's squared outputs are quadratic forms of its base values, so render_bwd forms per-instance
    // second moments and gauss_bwd_mom applies the forms per Gaussian (gsr_backward_power.hip).  Outputs
    // not requested (NULL) are skipped; dmeans3D is always formed.
    int moments() {
        const bool sh = g.shs != nullptr;
        if (sh && (cam.sh_degree < 0 || cam.sh_degree > 3))
            return fail(GSR_ERR_INVALID_ARG, "unsupported sh_degree for backward_power != 1");
        char* scratch;
        if (int rc = power_scratch(sizeof(float) * (size_t)moments_record_floats(sh) * (size_t)R, &scratch)) return rc;
        float* rec = (float*)scratch;
        hipError_t e;
        if (R > 0) {
            StageTimer t(GSR_STAGE_RENDER_BWD, R, stream);
            if ((e = launch_render_bwd_moments(cam, img.ranges, point_list, geo, img.final_T, img.n_contrib,
                                               c.dL_dout_color, sh, rec, guard, stream)) != hipSuccess)
                return hip_fail(e, "render backward (moments)");
        }
        StageTimer t(GSR_STAGE_GAUSS_BWD, P, stream);
        if ((e = launch_gauss_bwd_moments(cam, g, geo, c.radii, rec, out, guard, stream)) != hipSuccess)
            return hip_fail(e, "gaussian backward (moments)");
        return GSR_OK;
    }

    // per-pair powf before summation (renderCUDAFused, backward.cu:850-1140): gsr_backward_power.hip
    int general_power() {
        if (!out.dmeans2D || !out.dcolors || !out.dopacity || !out.dcov3D || !out.dscales || !out.drot)
            return fail(GSR_ERR_INVALID_ARG, "backward_power != 1 needs every gradient output pointer, or only "
                                             "dmeans3D (+ dopacity)");
        const int nsh = g.shs ? (cam.sh_degree + 1) * (cam.sh_degree + 1) : 0;
        const int nvp = power_record_floats(nsh);
        if (nvp < 0) return fail(GSR_ERR_INVALID_ARG, "unsupported sh_degree for backward_power != 1");
        const size_t jac_bytes = (sizeof(float) * JAC_FLOATS * (size_t)P + 255) / 256 * 256;
        char* scratch;
        if (int rc = power_scratch(jac_bytes + sizeof(float) * (size_t)nvp * (size_t)R, &scratch)) return rc;
        float* jac = (float*)scratch;
        float* rec = (float*)(scratch + jac_bytes);
        hipError_t e;
        {
            StageTimer t(GSR_STAGE_GAUSS_BWD, P, stream);
            if ((e = launch_gauss_jac(cam, g, geo, c.radii, jac, stream)) != hipSuccess)
                return hip_fail(e, "gaussian jacobian");
        }
        if (R > 0) {
            StageTimer t(GSR_STAGE_RENDER_BWD, R, stream);
            if ((e = launch_render_bwd_power(cam, g, img.ranges, point_list, geo, jac, img.final_T, img.n_contrib,
                                             c.dL_dout_color, c.power, rec, guard, stream)) != hipSuccess)
                return hip_fail(e, "render backward (power)");
        }
        StageTimer t(GSR_STAGE_GAUSS_BWD, P, stream);
        if ((e = launch_gauss_bwd_power(cam, g, geo, c.radii, rec, out, guard, stream)) != hipSuccess)
            return hip_fail(e, "gaussian backward (power)");
        return GSR_OK;
    }

    int power1() {
        const PoseFuse* pose = c.pose;
        // SH colours feed dL/dmeans3D through the view direction, so their sums are needed with SH
        // pose-fused tracking backward: the pose needs the geometric sums and the depth colours only
        const unsigned need =
            pose ? (NEED_COLORS2 | NEED_DL2_CH0_ONLY)
                 : (out.dopacity ? NEED_OPACITY : 0u) | ((out.dcolors || g.shs) ? NEED_COLORS : 0u) |
                       (c.dcolors2 ? NEED_COLORS2 : 0u) | (c.dl2_channels == 1 ? NEED_DL2_CH0_ONLY : 0u);
        RecLayout rec = bwd_rec_layout(need, c.colors2 != nullptr);
        // gsr_backward_dual_m2d: the mapping variant's record with the first colour set's (hx, hy) behind it
        constexpr unsigned kMapNeed = NEED_OPACITY | NEED_COLORS | NEED_COLORS2 | NEED_DL2_CH0_ONLY;
        M2dOut m1;
        if (c.dmeans2D_c1) {
            if (need != kMapNeed || !c.colors2 || pose || c.pre_inst || rec.stride != M2D_REC_PAIR)
                return fail(GSR_ERR_INVALID_ARG, "backward_dual_m2d: the mapping form only");
            m1.dmeans2D_c1 = c.dmeans2D_c1;
            m1.o_m1 = M2D_REC_PAIR;
            rec.stride = m2d_record_stride();
        }
        // staged SH backward: gauss_bwd leaves dL/dcolor in a scratch array, sh_bwd turns it into dsh and the
        // view-direction term of dL/dmeans3D (gsr_sh.hip)
        const bool shs_staged = sh_staged(cam, g);
        // pre_inst: the records were formed by the fused tracking render (render_track_kernel)
        const size_t rec_bytes =
            (c.pre_inst || R <= 0) ? 0 : align_up(sizeof(float) * rec.stride * (size_t)R, 256);
        // (a caller who asked for dL/dcolor with SH input gets it, as from the per-lane chain: gauss_bwd then
        // writes it straight into the caller's array, sh_bwd reads it from there and no scratch copy is reserved)
        const bool own_drgb = shs_staged && !out.dcolors;
        const size_t scratch_bytes = rec_bytes + (own_drgb ? sizeof(float) * 3 * (size_t)P : 0);
        char* scratch = nullptr;
        if (scratch_bytes > 0) {
            if (!c.alloc) return fail(GSR_ERR_INVALID_ARG, "allocator callback required");
            if (int rc = obtain(c.alloc, c.alloc_ctx, GSR_BUF_SCRATCH, scratch_bytes, "backward scratch", &scratch))
                return rc;
        }
        float* drgb = !shs_staged ? nullptr : own_drgb ? (float*)(scratch + rec_bytes) : out.dcolors;
        float* inst = nullptr;
        hipError_t e;
        if (c.pre_inst) {
            if (!pose || rec.stride != track_records_stride())
                return fail(GSR_ERR_INVALID_ARG, "precomputed records are the pose-fused tracking backward's only");
            inst = const_cast<float*>(c.pre_inst);
        } else if (R > 0) {
            if (!c.binning_buffer) return fail(GSR_ERR_INVALID_ARG, "missing binning buffer");
            inst = (float*)scratch;
            StageTimer t(GSR_STAGE_RENDER_BWD, R, stream, true);
            e = m1.dmeans2D_c1
                    ? launch_render_bwd_m2d(cam, img.ranges, point_list, geo, img.final_T, img.n_contrib,
                                            c.dL_dout_color, c.dL_dout_color2, inst, guard, stream, t.kclock())
                    : launch_render_bwd(cam, img.ranges, point_list, geo, img.final_T, img.n_contrib, c.dL_dout_color,
                                        c.colors2, c.dL_dout_color2, need, inst, guard, stream, t.kclock());
            if (e != hipSuccess) return hip_fail(e, "render backward");
        }
        out.dcolors2 = c.dcolors2;
        // (device-clock mode: gauss_bwd_kernel stamps itself; a staged sh_bwd after it is not timed)
        StageTimer t(GSR_STAGE_GAUSS_BWD, P, stream, true);
        GaussIn gc = g;
        GradsOut oc = out;
        if (shs_staged) {  // the chain without SH: dL/dcolor to scratch, dsh by sh_bwd below
            gc.shs = nullptr;
            gc.M = 0;
            oc.dcolors = drgb;
            oc.dsh = nullptr;
        }
        PoseFuse pc;
        if (pose) {
            pc = *pose;
            pc.guard = geo.counters;
        }
        e = m1.dmeans2D_c1
                ? launch_gauss_bwd_m2d(cam, gc, geo, c.radii, inst, rec, oc, m1, guard, stream, t.kclock())
                : launch_gauss_bwd(cam, gc, geo, c.radii, inst, rec, oc, guard, stream, pose ? &pc : nullptr,
                                   t.kclock());
        if (e != hipSuccess) return hip_fail(e, "gaussian backward");
        // the colour step guards on this call's own forward counters (not a sticky status row: an
        // overflow in an earlier replay must not skip the steps of later valid iterations)
        ShAdam sa = c.sh_adam ? *c.sh_adam : ShAdam{};
        if (c.sh_adam) {
            sa.guard = geo.counters;
            sa.cap = (uint32_t)R;
        }
        if (shs_staged && (e = launch_sh_bwd(cam, g, geo, c.radii, drgb, out.dmeans3D, out.dsh, guard, stream, sa)) !=
                              hipSuccess)
            return hip_fail(e, "sh backward");
        return GSR_OK;
    }
};

int backward_impl(const BwdCall& c) {
    const int rc = validate(c.settings, c.gaussians, false);
    if (c.dl2_channels != 1 && c.dl2_channels != 3) return fail(GSR_ERR_INVALID_ARG, "dl2_channels must be 1 or 3");
    if (rc != GSR_OK) return rc;
    // (with pre-formed records -- the fused tracking render's -- the gradient images are not read)
    if (c.colors2 && !c.dL_dout_color2 && !c.pre_inst)
        return fail(GSR_ERR_INVALID_ARG, "dual backward needs dL_dout_color2");
    if (c.colors2 && c.power != 1) return fail(GSR_ERR_INVALID_ARG, "dual render supports backward_power == 1 only");
    if (!c.grads) return fail(GSR_ERR_INVALID_ARG, "grads required");
    if (c.num_rendered < 0) return fail(GSR_ERR_INVALID_ARG, "num_rendered must be >= 0");
    Backward B(c);
    if (c.sh_adam && (c.power != 1 || !sh_staged(B.cam, B.g)))  // checked before any work is enqueued
        return fail(GSR_ERR_INVALID_ARG, "sh_adam needs staged SH colours (M == (D+1)^2) and power 1");
    if (B.P == 0) return GSR_OK;
    if (!c.geom_buffer || !c.image_buffer || !c.radii || (!c.dL_dout_color && !c.pre_inst))
        return fail(GSR_ERR_INVALID_ARG, "missing forward state");
    B.bind_forward_state();
    const GradsOut& o = B.out;
    if (!o.dmeans3D && !c.pose) return fail(GSR_ERR_INVALID_ARG, "dmeans3D output pointer required");
    if (c.power != 1 && !o.dmeans2D && !o.dcolors && !o.dcov3D && !o.dscales && !o.drot && !o.dsh) return B.fisher();
    if (c.power == 2) return B.moments();
    if (c.power != 1) return B.general_power();
    return B.power1();
}

// The two forwards that run the tracking transform inside preprocess check their gsr_track_xform alike, under
// their own names.  mapping (gsr_forward_dual_static_xf): store_rendervars must be set, the RGB colours are
// required, and SH / cov3D are reported before a null pointer -- the tracking entry reports them after.
int check_xform(const char* entry, const FwdCall& c, const gsr_track_xform* xform, bool mapping) {
    const gsr_gaussians* g = c.gaussians;
    auto refuse = [entry](const char* what) { return fail(GSR_ERR_INVALID_ARG, std::string(entry) + ": " + what); };
    if (!xform || !g) return refuse("null pointer");
    const gsr_track_xform& x = *xform;
    if ((x.scale_cols != 1 && x.scale_cols != 3) || x.q_stride < 1)
        return refuse("bad sizes");
    if (mapping && !x.store_rendervars) return refuse("store_rendervars must be 1");
    const void* colour = mapping ? g->colors_precomp : c.colors2;
    const bool null_pointer =
        g->P > 0 && (!x.means_world || !x.unnorm_rot || !x.logit_opac || !x.log_scales || !x.cam_q || !x.cam_t ||
                     !x.w2c || !g->means3D || !g->rotations || !g->opacities || !g->scales || !colour);
    if (!mapping && null_pointer) return refuse("null pointer");
    if (g->shs || g->cov3D_precomp) return refuse("precomputed colours, scales / rotations only");
    if (null_pointer) return refuse("null pointer");
    if (!c.colors2) return fail(GSR_ERR_INVALID_ARG, "colors2 required");
    if (c.capacity <= 0 || !c.status) return fail(GSR_ERR_INVALID_ARG, "static mode needs capacity > 0 and status");
    return GSR_OK;
}

TrackXf make_xf(const gsr_track_xform& x) {
    TrackXf xf;
    xf.mw = x.means_world; xf.ur = x.unnorm_rot; xf.lo = x.logit_opac; xf.ls = x.log_scales;
    xf.scols = x.scale_cols; xf.cq = x.cam_q; xf.ct = x.cam_t; xf.qs = x.q_stride; xf.w2c = x.w2c;
    xf.store = x.store_rendervars != 0;
    return xf;
}

// gsr_track_forward_dual_static_xf, and with c.track_inst the fused forward + backward (which forms no
// gradient images: l1.dL_dim / dL_dds NULL)
int track_forward_xf(FwdCall c, const gsr_track_xform* xform, const TrackL1& l1) {
    if (int rc = check_xform("track_forward_dual_static_xf", c, xform, false)) return rc;
    if (!l1.gt_im || !l1.gt_depth || !l1.seed || !l1.loss || (!c.track_inst && (!l1.dL_dim || !l1.dL_dds)) ||
        !l1.scratch)
        return fail(GSR_ERR_INVALID_ARG, "track_forward_dual_static_xf: null pointer");
    const TrackXf xf = make_xf(*xform);
    c.l1 = &l1;
    c.xf = &xf;
    c.alive = xform->alive;
    return forward_impl(c);
}

// gsr_track_backward_dual(_records): c holds the forward state (and the gradient images or the records), pf
// the entry's pose arguments
int track_backward(BwdCall c, PoseFuse pf, const gsr_pose_track* track, const float* log_scales) {
    if (!c.gaussians || (pf.scols != 1 && pf.scols != 3) || pf.qs < 1)
        return fail(GSR_ERR_INVALID_ARG, "track_backward_dual: bad sizes");
    if (!c.colors2 || !pf.means_world || !pf.unnorm_rot || !pf.cam_q || !pf.cam_t || !pf.w2c || !pf.scratch ||
        (!pf.adam_state && (!pf.dq || !pf.dt)))
        return fail(GSR_ERR_INVALID_ARG, "track_backward_dual: null pointer");
    if (pf.scols != 1 && !c.gaussians->rotations)
        return fail(GSR_ERR_INVALID_ARG, "track_backward_dual: anisotropic maps need the rendered rotations");
    pf.cap = (uint32_t)c.num_rendered;  // pf.guard = the forward's counters (Backward::power1)
    pf.ls = log_scales;                 // recompute the rendervars (forward without stored rendervars)
    if (track) {
        pf.loss = track->loss;
        pf.best = track->best;
    }
    const gsr_grads none{};
    c.grads = &none;
    c.dl2_channels = 1;
    c.pose = &pf;
    return backward_impl(c);
}

}  // namespace

extern "C" {

int gsr_abi_version(void) { return GSR_ABI_VERSION; }

const char* gsr_last_error(void) { return g_last_error.c_str(); }

size_t gsr_geom_buffer_bytes(int P) { return GeomLayout::make(P).total; }
size_t gsr_geom_counters_offset(int P) { return GeomLayout::make(P).counters; }
size_t gsr_binning_buffer_bytes(int num_rendered, int W, int H) { return BinLayout::make(num_rendered, W, H).total; }
size_t gsr_image_buffer_bytes(int W, int H) { return ImgLayout::make(W, H).total; }

int gsr_forward(const gsr_settings* settings, const gsr_gaussians* gaussians, float* out_color, float* out_depth,
                int* radii, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    return forward_impl(fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream));
}

int gsr_forward_dual(const gsr_settings* settings, const gsr_gaussians* gaussians, const float* colors2,
                     float* out_color, float* out_color2, float* out_depth, int* radii, gsr_alloc_fn alloc,
                     void* alloc_ctx, void* stream) {
    if (!colors2) return fail(GSR_ERR_INVALID_ARG, "colors2 required");
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    return forward_impl(dual(c, colors2, out_color2));
}

int gsr_forward_static(const gsr_settings* settings, const gsr_gaussians* gaussians, int capacity, unsigned* status,
                       float* out_color, float* out_depth, int* radii, gsr_alloc_fn alloc, void* alloc_ctx,
                       void* stream) {
    if (capacity <= 0 || !status) return fail(GSR_ERR_INVALID_ARG, "static mode needs capacity > 0 and status");
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    return forward_impl(statics(c, capacity, status));
}

// the checks every static dual entry makes first
static int check_dual_static(const float* colors2, int capacity, const unsigned* status) {
    if (!colors2) return fail(GSR_ERR_INVALID_ARG, "colors2 required");
    if (capacity <= 0 || !status) return fail(GSR_ERR_INVALID_ARG, "static mode needs capacity > 0 and status");
    return GSR_OK;
}

int gsr_forward_dual_static(const gsr_settings* settings, const gsr_gaussians* gaussians, const float* colors2,
                            int capacity, unsigned* status, float* out_color, float* out_color2, float* out_depth,
                            int* radii, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    if (int rc = check_dual_static(colors2, capacity, status)) return rc;
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    return forward_impl(statics(dual(c, colors2, out_color2), capacity, status));
}

int gsr_forward_dual_static_alive(const gsr_settings* settings, const gsr_gaussians* gaussians, const float* colors2,
                                  int capacity, unsigned* status, float* out_color, float* out_color2,
                                  float* out_depth, int* radii, const unsigned char* alive, gsr_alloc_fn alloc,
                                  void* alloc_ctx, void* stream) {
    if (int rc = check_dual_static(colors2, capacity, status)) return rc;
    if (!alive && gaussians && gaussians->P > 0) return fail(GSR_ERR_INVALID_ARG, "alive mask required");
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    c.alive = alive;
    return forward_impl(statics(dual(c, colors2, out_color2), capacity, status));
}

int gsr_forward_static_alive(const gsr_settings* settings, const gsr_gaussians* gaussians, int capacity,
                             unsigned* status, float* out_color, float* out_depth, int* radii,
                             const unsigned char* alive, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    if (capacity <= 0 || !status) return fail(GSR_ERR_INVALID_ARG, "static mode needs capacity > 0 and status");
    if (!alive && gaussians && gaussians->P > 0) return fail(GSR_ERR_INVALID_ARG, "alive mask required");
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    c.alive = alive;
    return forward_impl(statics(c, capacity, status));
}

int gsr_forward_dual_static_xf(const gsr_settings* settings, const gsr_gaussians* gaussians, float* colors2,
                               const gsr_track_xform* xform, int capacity, unsigned* status, float* out_color,
                               float* out_color2, float* out_depth, int* radii, gsr_alloc_fn alloc, void* alloc_ctx,
                               void* stream) {
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    statics(dual(c, colors2, out_color2), capacity, status);
    if (int rc = check_xform("forward_dual_static_xf", c, xform, true)) return rc;
    const TrackXf xf = make_xf(*xform);
    c.xf = &xf;
    c.alive = xform->alive;
    return forward_impl(c);
}

int gsr_track_forward_scratch_floats(int image_width, int image_height) {
    const int gx = (image_width + TILE_X - 1) / TILE_X, gy = (image_height + TILE_Y - 1) / TILE_Y;
    return track_l1_fused_scratch_floats(gx * gy > 0 ? gx * gy : 1);
}

// The three tracking forwards and their _terms siblings share one body each: `terms` NULL is the entry without
// them (the kernels then take today's path), and a sibling's own check (check_terms) comes before the shared ones.
static int track_forward_static(FwdCall c, const float* colors2, float* out_color2, int capacity, unsigned* status,
                                const TrackL1& l1) {
    if (int rc = check_dual_static(colors2, capacity, status)) return rc;
    if (!l1.gt_im || !l1.gt_depth || !l1.seed || !l1.loss || !l1.dL_dim || !l1.dL_dds || !l1.scratch)
        return fail(GSR_ERR_INVALID_ARG, "track_forward_dual_static: null pointer");
    c.l1 = &l1;
    return forward_impl(statics(dual(c, colors2, out_color2), capacity, status));
}

int gsr_track_forward_dual_static(const gsr_settings* settings, const gsr_gaussians* gaussians, const float* colors2,
                                  int capacity, unsigned* status, float* out_color, float* out_color2,
                                  float* out_depth, int* radii, const float* gt_im, const float* gt_depth,
                                  float sil_thres, float w_im, float w_depth, const float* dL_dloss, float* loss,
                                  float* dL_dim, float* dL_ddepth_sil, float* scratch, gsr_alloc_fn alloc,
                                  void* alloc_ctx, void* stream) {
    return track_forward_static(
        fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream), colors2, out_color2,
        capacity, status,
        TrackL1{gt_im, gt_depth, sil_thres, w_im, w_depth, dL_dloss, dL_dim, dL_ddepth_sil, scratch, loss, nullptr});
}

int gsr_track_forward_dual_static_terms(const gsr_settings* settings, const gsr_gaussians* gaussians,
                                        const float* colors2, int capacity, unsigned* status, float* out_color,
                                        float* out_color2, float* out_depth, int* radii, const float* gt_im,
                                        const float* gt_depth, float sil_thres, float w_im, float w_depth,
                                        const float* dL_dloss, float* loss, float* terms, float* dL_dim,
                                        float* dL_ddepth_sil, float* scratch, gsr_alloc_fn alloc, void* alloc_ctx,
                                        void* stream) {
    if (int rc = check_terms("track_forward_dual_static_terms", terms)) return rc;
    return track_forward_static(
        fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream), colors2, out_color2,
        capacity, status,
        TrackL1{gt_im, gt_depth, sil_thres, w_im, w_depth, dL_dloss, dL_dim, dL_ddepth_sil, scratch, loss, terms});
}

int gsr_track_forward_dual_static_xf(const gsr_settings* settings, const gsr_gaussians* gaussians, float* colors2,
                                     const gsr_track_xform* xform, int capacity, unsigned* status, float* out_color,
                                     float* out_color2, float* out_depth, int* radii, const float* gt_im,
                                     const float* gt_depth, float sil_thres, float w_im, float w_depth,
                                     const float* dL_dloss, float* loss, float* dL_dim, float* dL_ddepth_sil,
                                     float* scratch, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    statics(dual(c, colors2, out_color2), capacity, status);
    return track_forward_xf(c, xform,
                            TrackL1{gt_im, gt_depth, sil_thres, w_im, w_depth, dL_dloss, dL_dim, dL_ddepth_sil,
                                    scratch, loss, nullptr});
}

int gsr_track_forward_dual_static_xf_terms(const gsr_settings* settings, const gsr_gaussians* gaussians,
                                           float* colors2, const gsr_track_xform* xform, int capacity,
                                           unsigned* status, float* out_color, float* out_color2, float* out_depth,
                                           int* radii, const float* gt_im, const float* gt_depth, float sil_thres,
                                           float w_im, float w_depth, const float* dL_dloss, float* loss,
                                           float* terms, float* dL_dim, float* dL_ddepth_sil, float* scratch,
                                           gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    if (int rc = check_terms("track_forward_dual_static_xf_terms", terms)) return rc;
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    statics(dual(c, colors2, out_color2), capacity, status);
    return track_forward_xf(c, xform,
                            TrackL1{gt_im, gt_depth, sil_thres, w_im, w_depth, dL_dloss, dL_dim, dL_ddepth_sil,
                                    scratch, loss, terms});
}

int gsr_track_records_floats(int capacity) { return track_records_stride() * (capacity > 1 ? capacity : 1); }

// gsr_track_forward_backward_dual_static_xf(_terms)
static int track_forward_backward_xf(FwdCall c, float* colors2, float* out_color2, const gsr_track_xform* xform,
                                     int capacity, unsigned* status, float* inst_records, const TrackL1& l1) {
    if (!inst_records) return fail(GSR_ERR_INVALID_ARG, "track_forward_backward_dual_static_xf: null records");
    // the gradient images are not formed (the backward runs from the registers); the L1 epilogue's
    // pointers to them are never dereferenced.  out_color, out_color2 and out_depth all NULL: the rendered
    // images (and final_T / n_contrib / the block maxima of the image buffer) are not stored either
    statics(dual(c, colors2, out_color2), capacity, status).track_inst = inst_records;
    return track_forward_xf(c, xform, l1);
}

int gsr_track_forward_backward_dual_static_xf(const gsr_settings* settings, const gsr_gaussians* gaussians,
                                              float* colors2, const gsr_track_xform* xform, int capacity,
                                              unsigned* status, float* out_color, float* out_color2,
                                              float* out_depth, int* radii, const float* gt_im,
                                              const float* gt_depth, float sil_thres, float w_im, float w_depth,
                                              const float* dL_dloss, float* loss, float* scratch,
                                              float* inst_records, gsr_alloc_fn alloc, void* alloc_ctx,
                                              void* stream) {
    return track_forward_backward_xf(
        fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream), colors2, out_color2,
        xform, capacity, status, inst_records,
        TrackL1{gt_im, gt_depth, sil_thres, w_im, w_depth, dL_dloss, nullptr, nullptr, scratch, loss, nullptr});
}

int gsr_track_forward_backward_dual_static_xf_terms(const gsr_settings* settings, const gsr_gaussians* gaussians,
                                                    float* colors2, const gsr_track_xform* xform, int capacity,
                                                    unsigned* status, float* out_color, float* out_color2,
                                                    float* out_depth, int* radii, const float* gt_im,
                                                    const float* gt_depth, float sil_thres, float w_im,
                                                    float w_depth, const float* dL_dloss, float* loss, float* terms,
                                                    float* scratch, float* inst_records, gsr_alloc_fn alloc,
                                                    void* alloc_ctx, void* stream) {
    if (int rc = check_terms("track_forward_backward_dual_static_xf_terms", terms)) return rc;
    return track_forward_backward_xf(
        fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream), colors2, out_color2,
        xform, capacity, status, inst_records,
        TrackL1{gt_im, gt_depth, sil_thres, w_im, w_depth, dL_dloss, nullptr, nullptr, scratch, loss, terms});
}

int gsr_forward_reuse(const gsr_settings* settings, const gsr_gaussians* gaussians, int num_rendered,
                      const void* prev_geom, void* binning_buffer, void* image_buffer, const int* prev_radii,
                      float* out_color, float* out_depth, int* radii, gsr_alloc_fn alloc, void* alloc_ctx,
                      void* stream_) {
    int rc = validate(settings, gaussians, true);
    if (rc != GSR_OK) return rc;
    if (!alloc) return fail(GSR_ERR_INVALID_ARG, "allocator callback required");
    if (!gaussians->colors_precomp || (gaussians->shs && gaussians->M > 0))
        return fail(GSR_ERR_INVALID_ARG, "geometry reuse needs precomputed colours (no SH)");
    if (gaussians->P <= 0 || num_rendered < 0 || !prev_geom || !binning_buffer || !image_buffer || !prev_radii ||
        !out_color || !out_depth || !radii)
        return fail(GSR_ERR_INVALID_ARG, "geometry reuse needs the previous call's state and the outputs");
    hipStream_t stream = (hipStream_t)stream_;
    const int dev = stream_device(stream);
    Camera cam = make_camera(settings);
    const GaussIn g = make_gauss(gaussians);
    const int P = g.P;
    const GeomLayout GL = GeomLayout::make(P);
    cam.pre_shift = GL.shift;
    void* geom;
    if ((rc = obtain(alloc, alloc_ctx, GSR_BUF_GEOM, GL.total, "geom buffer", &geom)) != GSR_OK) return rc;
    const GeomPtrs geo = GeomPtrs::at(geom, GL);
    const ImgPtrs img = ImgPtrs::at(image_buffer, ImgLayout::make(cam.W, cam.H));
    bind_schedule(cam, img, dev);
    hipError_t e;
    {
        StageTimer t(GSR_STAGE_PREPROCESS, P, stream);
        if ((e = hipMemcpyAsync(geom, prev_geom, GL.total, hipMemcpyDeviceToDevice, stream)) != hipSuccess ||
            (e = hipMemcpyAsync(radii, prev_radii, sizeof(int) * (size_t)P, hipMemcpyDeviceToDevice, stream)) !=
                hipSuccess)
            return hip_fail(e, "copy previous geometry");
        if ((e = launch_recolour(P, g.colors, geo, stream)) != hipSuccess) return hip_fail(e, "recolour");
    }
    // the previous render_fwd left point_list sorted (with its block masks): no sort, any list length
    const SpecGuard guard{geo.counters, (uint32_t)num_rendered, 0xFFFFFFFFu};
    StageTimer t(GSR_STAGE_RENDER_FWD, num_rendered, stream, true);
    if ((e = launch_render_fwd(cam, img.ranges, (uint64_t*)binning_buffer, nullptr, geo, nullptr, img.final_T,
                               img.n_contrib, out_color, nullptr, out_depth, guard, stream, t.kclock())) != hipSuccess)
        return hip_fail(e, "render");
    return num_rendered;
}

int gsr_forward_reuse_if_equal(const gsr_settings* settings, const gsr_gaussians* gaussians, int npairs,
                               const float* const* a, const float* const* b, const long long* n,
                               int prev_num_rendered, const void* prev_geom, void* prev_binning, void* prev_image,
                               const int* prev_radii, float* out_color, float* out_depth, int* radii, int* reused,
                               gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    if (!gaussians || !gaussians->colors_precomp || (gaussians->shs && gaussians->M > 0) || gaussians->cov3D_precomp)
        return fail(GSR_ERR_INVALID_ARG, "geometry reuse needs precomputed colours (no SH, no cov3D)");
    if (npairs < 1 || npairs > 8 || !a || !b || !n || !reused)
        return fail(GSR_ERR_INVALID_ARG, "gsr_forward_reuse_if_equal: 1..8 pairs and `reused`");
    if (prev_num_rendered < 0 || !prev_geom || !prev_binning || !prev_image || !prev_radii)
        return fail(GSR_ERR_INVALID_ARG, "geometry reuse needs the previous call's state");
    ReuseIn r{};
    r.pairs.npairs = npairs;
    for (int k = 0; k < npairs; k++) {
        if (n[k] < 0 || (n[k] > 0 && (!a[k] || !b[k])))
            return fail(GSR_ERR_INVALID_ARG, "gsr_forward_reuse_if_equal: pair");
        r.pairs.a[k] = a[k];
        r.pairs.b[k] = b[k];
        r.pairs.n[k] = n[k];
    }
    r.prev_num_rendered = prev_num_rendered;
    r.prev_geom = prev_geom;
    r.prev_binning = prev_binning;
    r.prev_image = prev_image;
    r.prev_radii = prev_radii;
    r.reused = reused;
    FwdCall c = fwd_call(settings, gaussians, out_color, out_depth, radii, alloc, alloc_ctx, stream);
    c.reuse = &r;
    return forward_impl(c);
}

int gsr_bitwise_equal(int npairs, const float* const* a, const float* const* b, const long long* n, int* flag,
                      void* stream) {
    if (npairs < 0 || npairs > 8 || (npairs > 0 && (!a || !b || !n)) || !flag)
        return fail(GSR_ERR_INVALID_ARG, "gsr_bitwise_equal: 0..8 pairs and a flag");
    EqualPairs q{};
    q.npairs = npairs;
    for (int k = 0; k < npairs; k++) {
        if (n[k] < 0 || (n[k] > 0 && (!a[k] || !b[k]))) return fail(GSR_ERR_INVALID_ARG, "gsr_bitwise_equal: pair");
        q.a[k] = a[k];
        q.b[k] = b[k];
        q.n[k] = n[k];
    }
    hipError_t e = zero_async(flag, sizeof(int), (hipStream_t)stream);  // (kernel: valid under capture too)
    if (e == hipSuccess) e = launch_bitwise_equal(q, flag, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "bitwise_equal");
    return GSR_OK;
}

int gsr_backward(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                 const float* dL_dout_color, int num_rendered, const void* geom_buffer, const void* binning_buffer,
                 const void* image_buffer, int power, const gsr_grads* grads, gsr_alloc_fn alloc, void* alloc_ctx,
                 void* stream) {
    BwdCall c = bwd_call(settings, gaussians, radii, num_rendered, geom_buffer, binning_buffer, image_buffer);
    c.dL_dout_color = dL_dout_color; c.power = power; c.grads = grads;
    return backward_impl(on(c, alloc, alloc_ctx, stream));
}

int gsr_backward_dual(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                      const float* colors2, const float* dL_dout_color, const float* dL_dout_color2,
                      int num_rendered, const void* geom_buffer, const void* binning_buffer,
                      const void* image_buffer, const gsr_grads* grads, float* dcolors2, int dl2_channels,
                      gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    if (!colors2) return fail(GSR_ERR_INVALID_ARG, "colors2 required");
    BwdCall c = bwd_call(settings, gaussians, radii, num_rendered, geom_buffer, binning_buffer, image_buffer);
    c.colors2 = colors2; c.dL_dout_color = dL_dout_color; c.dL_dout_color2 = dL_dout_color2;
    c.grads = grads; c.dcolors2 = dcolors2; c.dl2_channels = dl2_channels;
    return backward_impl(on(c, alloc, alloc_ctx, stream));
}

int gsr_backward_dual_m2d(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                          const float* colors2, const float* dL_dout_color, const float* dL_dout_color2,
                          int num_rendered, const void* geom_buffer, const void* binning_buffer,
                          const void* image_buffer, const gsr_grads* grads, float* dcolors2, int dl2_channels,
                          float* dmeans2D_color1, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    // the sibling's own checks come before the shared ones (like check_terms for the _terms entries)
    if (!dmeans2D_color1) return fail(GSR_ERR_INVALID_ARG, "backward_dual_m2d: dmeans2D_color1 must not be NULL");
    if ((uintptr_t)dmeans2D_color1 % 4 != 0)
        return fail(GSR_ERR_INVALID_ARG, "backward_dual_m2d: dmeans2D_color1 must be 4-byte aligned");
    if (!colors2) return fail(GSR_ERR_INVALID_ARG, "colors2 required");
    if (dl2_channels != 1) return fail(GSR_ERR_INVALID_ARG, "backward_dual_m2d: dl2_channels must be 1");
    if (!grads || !grads->dopacity || !dcolors2 || (!grads->dcolors && !(gaussians && gaussians->shs)))
        return fail(GSR_ERR_INVALID_ARG, "backward_dual_m2d: the mapping form only (dopacity, dcolors2 and dcolors "
                                         "or SH colours)");
    BwdCall c = bwd_call(settings, gaussians, radii, num_rendered, geom_buffer, binning_buffer, image_buffer);
    c.colors2 = colors2; c.dL_dout_color = dL_dout_color; c.dL_dout_color2 = dL_dout_color2;
    c.grads = grads; c.dcolors2 = dcolors2; c.dl2_channels = dl2_channels; c.dmeans2D_c1 = dmeans2D_color1;
    return backward_impl(on(c, alloc, alloc_ctx, stream));
}

int gsr_backward_dual_sh_adam(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                              const float* colors2, const float* dL_dout_color, const float* dL_dout_color2,
                              int num_rendered, const void* geom_buffer, const void* binning_buffer,
                              const void* image_buffer, const gsr_grads* grads, float* dcolors2, int dl2_channels,
                              const gsr_map_adam* sh_adam, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    if (!colors2) return fail(GSR_ERR_INVALID_ARG, "colors2 required");
    if (!sh_adam || !gaussians || !gaussians->shs || sh_adam->step < 1 || !sh_adam->exp_avg[4] ||
        !sh_adam->exp_avg_sq[4])
        return fail(GSR_ERR_INVALID_ARG, "backward_dual_sh_adam: SH colours and the colour group's state required");
    // the scalars exactly as gsr_map_transform_bwd_adam forms them (python floats -> float)
    ShAdam sa;
    sa.m = sh_adam->exp_avg[4];
    sa.v = sh_adam->exp_avg_sq[4];
    sa.ss = (float)(-sh_adam->lr[4] / adam_bc1(sh_adam->beta1, sh_adam->step));
    sa.c = adam_coef(sh_adam->beta1, sh_adam->beta2, sh_adam->eps, sh_adam->step);
    sa.halted = sh_adam->halted;
    // sa.guard / sa.cap: the forward's own counters (Backward::power1); sh_adam->status is not read
    BwdCall c = bwd_call(settings, gaussians, radii, num_rendered, geom_buffer, binning_buffer, image_buffer);
    c.colors2 = colors2; c.dL_dout_color = dL_dout_color; c.dL_dout_color2 = dL_dout_color2;
    c.grads = grads; c.dcolors2 = dcolors2; c.dl2_channels = dl2_channels; c.sh_adam = &sa;
    return backward_impl(on(c, alloc, alloc_ctx, stream));
}

int gsr_track_backward_scratch_floats(int P) { return pose_fuse_scratch_floats(P < 1 ? 1 : P); }

int gsr_track_backward_dual(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                            const float* colors2, const float* dL_dout_color, const float* dL_dout_color2,
                            int num_rendered, const void* geom_buffer, const void* binning_buffer,
                            const void* image_buffer, const float* means_world, const float* unnorm_rot,
                            int scale_cols, float* cam_q, float* cam_t, int q_stride, const float* w2c, double lr_q,
                            double lr_t, double beta1, double beta2, double eps, float* adam_state,
                            float* dL_dcam_q, float* dL_dcam_t, float* scratch, const gsr_pose_track* track,
                            const float* log_scales, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    BwdCall c = bwd_call(settings, gaussians, radii, num_rendered, geom_buffer, binning_buffer, image_buffer);
    c.colors2 = colors2; c.dL_dout_color = dL_dout_color; c.dL_dout_color2 = dL_dout_color2;
    on(c, alloc, alloc_ctx, stream);
    const PoseFuse pf{means_world, unnorm_rot, scale_cols, cam_q, cam_t, q_stride, w2c, scratch, adam_state,
                      lr_q, lr_t, beta1, beta2, eps, dL_dcam_q, dL_dcam_t};
    return track_backward(c, pf, track, log_scales);
}

int gsr_track_backward_dual_records(const gsr_settings* settings, const gsr_gaussians* gaussians, const int* radii,
                                    const float* colors2, int num_rendered, const void* geom_buffer,
                                    const void* binning_buffer, const void* image_buffer, const float* means_world,
                                    const float* unnorm_rot, int scale_cols, float* cam_q, float* cam_t, int q_stride,
                                    const float* w2c, double lr_q, double lr_t, double beta1, double beta2,
                                    double eps, float* adam_state, float* dL_dcam_q, float* dL_dcam_t,
                                    float* scratch, const gsr_pose_track* track, const float* log_scales,
                                    const float* inst_records, gsr_alloc_fn alloc, void* alloc_ctx, void* stream) {
    if (!inst_records) return fail(GSR_ERR_INVALID_ARG, "track_backward_dual_records: null records");
    // (the gradient images are not read: the records already hold the render backward's sums)
    BwdCall c = bwd_call(settings, gaussians, radii, num_rendered, geom_buffer, binning_buffer, image_buffer);
    c.colors2 = colors2; c.pre_inst = inst_records;
    on(c, alloc, alloc_ctx, stream);
    const PoseFuse pf{means_world, unnorm_rot, scale_cols, cam_q, cam_t, q_stride, w2c, scratch, adam_state,
                      lr_q, lr_t, beta1, beta2, eps, dL_dcam_q, dL_dcam_t};
    return track_backward(c, pf, track, log_scales);
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* visible, void* stream) {
    (void)projmatrix;
    if (P < 0) return fail(GSR_ERR_INVALID_ARG, "P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrix || !visible) return fail(GSR_ERR_INVALID_ARG, "null pointer");
    hipError_t e = launch_mark_visible(P, means3D, viewmatrix, visible, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "mark_visible");
    return GSR_OK;
}

// Test hook: validates the wave64 permlane/DPP reduction on the device.
int gsr_selftest_reduce9(const float* in_dev, float* out_dev, void* stream) {
    hipError_t e = launch_selftest_reduce9(in_dev, out_dev, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "selftest");
    return GSR_OK;
}

}  // extern "C"
