// extern "C" driver over the reference's CudaRasterizer::Rasterizer, compiled by hipcc for gfx950
// together with the reference's own forward.cu / backward.cu / rasterizer_impl.cu (oracle/Makefile,
// target `ref`).  TEST INFRASTRUCTURE ONLY: loaded by oracle/reference.py through ctypes, never by
// the product.  The reference's entry points take device pointers and three std::function chunk
// allocators; this file owns every device allocation, checks every HIP status, validates sizes
// before anything is launched, and copies the forward's intermediate state out through the
// reference's own fromChunk (no offsets are derived here).
//
// Return codes: 0 success; > 0 a hipError_t; < 0 a refusal of this driver (REF_E_*).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <vector>

#include "rasterizer_impl.h"

namespace {

enum {
    REF_E_ARG = -1,      // a null or inconsistent argument, P <= 0 included
    REF_E_SIZE = -2,     // a size outside what the reference's int indexing holds
    REF_E_THROWN = -3,   // the reference (or a chunk allocator) threw
    REF_E_STATE = -4,    // backward / copy-out on a context whose forward did not complete
};

struct Chunk {
    char* ptr = nullptr;
    size_t size = 0;
};

struct Ctx {
    int P = 0, D = 0, M = 0, W = 0, H = 0, R = -1;
    float scale_modifier = 1.f, tan_fovx = 0.f, tan_fovy = 0.f;
    float *bg = nullptr, *means3D = nullptr, *shs = nullptr, *colors = nullptr, *opacities = nullptr,
          *scales = nullptr, *rotations = nullptr, *cov3D = nullptr, *view = nullptr, *proj = nullptr,
          *campos = nullptr, *out_color = nullptr, *out_depth = nullptr;
    int* radii = nullptr;
    Chunk geom, binning, img;
    std::vector<void*> owned;  // every hipMalloc of this context except the three chunks
    hipError_t alloc_err = hipSuccess;
};

#define REF_HIP(call)                      \
    do {                                   \
        hipError_t e_ = (call);            \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

int dev_alloc(Ctx* c, void** dst, size_t bytes) {
    *dst = nullptr;
    REF_HIP(hipMalloc(dst, bytes ? bytes : 4));
    c->owned.push_back(*dst);
    REF_HIP(hipMemset(*dst, 0, bytes ? bytes : 4));
    return 0;
}

// host -> device copy of n floats; a null host pointer stays a null device pointer
int upload(Ctx* c, float** dst, const float* host, size_t n) {
    *dst = nullptr;
    if (!host) return 0;
    int rc = dev_alloc(c, (void**)dst, n * sizeof(float));
    if (rc) return rc;
    REF_HIP(hipMemcpy(*dst, host, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

std::function<char*(size_t)> chunk_allocator(Ctx* c, Chunk* k) {
    return [c, k](size_t n) -> char* {
        if (k->ptr) {
            (void)hipFree(k->ptr);
            k->ptr = nullptr;
            k->size = 0;
        }
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) e = hipMemset(p, 0, n);
        if (e != hipSuccess) {  // the reference would write through the null pointer: stop it here
            c->alloc_err = e;
            if (p) (void)hipFree(p);
            throw std::runtime_error("chunk allocation failed");
        }
        k->ptr = (char*)p;
        k->size = n;
        return k->ptr;
    };
}

void release(Ctx* c) {
    for (void* p : c->owned) (void)hipFree(p);
    for (Chunk* k : {&c->geom, &c->binning, &c->img})
        if (k->ptr) (void)hipFree(k->ptr);
    delete c;
}

template <typename T>
int download(void* host, const T* dev, size_t n) {
    if (!host || n == 0) return 0;
    REF_HIP(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

struct RefIn {
    int P, D, M, W, H;
    const float *bg, *means3D, *shs, *colors, *opacities, *scales, *rotations, *cov3D_precomp;
    float scale_modifier;
    const float *view, *proj, *campos;
    float tan_fovx, tan_fovy;
};

// Host arrays the forward's results are copied to (any may be null: not copied).
struct RefFwdOut {
    float* out_color;         // [3,H,W]
    float* out_depth;         // [H,W]
    int* radii;               // [P]
    float* means2D;           // [P,2]
    float* depths;            // [P]
    float* conic_opacity;     // [P,4]
    float* rgb;               // [P,3]
    unsigned char* clamped;   // [P,3]
    int* tiles_touched;       // [P]
    float* final_T;           // [H,W]   ImageState::accum_alpha
    int* n_contrib;           // [H,W]
    int* ranges;              // [tiles,2]
    int num_rendered;         // written by ref_forward
};

struct RefGrads {
    float *dmeans2D, *dcolors, *dopacity, *dmeans3D, *dcov3D, *dsh, *dscales, *drot;  // shapes of rasterize_points.cu
};

const char* ref_strerror(int rc) {
    switch (rc) {
        case 0: return "success";
        case REF_E_ARG: return "ref_driver: null, empty or inconsistent argument";
        case REF_E_SIZE: return "ref_driver: size outside the reference's int indexing";
        case REF_E_THROWN: return "ref_driver: the reference or a chunk allocator threw";
        case REF_E_STATE: return "ref_driver: the context holds no completed forward";
    }
    return rc > 0 ? hipGetErrorString((hipError_t)rc) : "ref_driver: unknown code";
}

void ref_free(void* ctx) {
    if (ctx) release((Ctx*)ctx);
}

// The reference forward (prefiltered = false always).  On success *ctx_out owns the device state
// the backward and ref_point_list need; free it with ref_free.  Nothing is launched when an
// argument is refused.
int ref_forward(const RefIn* in, RefFwdOut* out, void** ctx_out) {
    if (!in || !out || !ctx_out) return REF_E_ARG;
    *ctx_out = nullptr;
    if (in->P <= 0 || in->W <= 0 || in->H <= 0 || in->D < 0 || in->D > 3 || in->M < 0) return REF_E_ARG;
    if (!in->bg || !in->means3D || !in->opacities || !in->view || !in->proj || !in->campos) return REF_E_ARG;
    if ((in->shs != nullptr) == (in->colors != nullptr)) return REF_E_ARG;  // exactly one colour source
    if (in->shs && (in->M < (in->D + 1) * (in->D + 1) || in->M > 64)) return REF_E_ARG;  // M stored >= the active (D+1)^2
    if (!in->shs && in->M != 0) return REF_E_ARG;
    if (in->cov3D_precomp ? (in->scales || in->rotations) : (!in->scales || !in->rotations)) return REF_E_ARG;
    if (!(in->tan_fovx > 0.f) || !(in->tan_fovy > 0.f)) return REF_E_ARG;
    if (in->P > (1 << 24) || (long long)in->W * in->H > (1 << 26) || in->W > (1 << 14) || in->H > (1 << 14))
        return REF_E_SIZE;

    Ctx* c = new Ctx;
    c->P = in->P; c->D = in->D; c->M = in->M; c->W = in->W; c->H = in->H;
    c->scale_modifier = in->scale_modifier; c->tan_fovx = in->tan_fovx; c->tan_fovy = in->tan_fovy;
    const size_t P = in->P, N = (size_t)in->W * in->H;
    int rc = 0;
#define REF_TRY(expr)             \
    if ((rc = (expr)) != 0) {     \
        release(c);               \
        return rc;                \
    }
    REF_TRY(upload(c, &c->bg, in->bg, 3));
    REF_TRY(upload(c, &c->means3D, in->means3D, P * 3));
    REF_TRY(upload(c, &c->shs, in->shs, P * in->M * 3));
    REF_TRY(upload(c, &c->colors, in->colors, P * 3));
    REF_TRY(upload(c, &c->opacities, in->opacities, P));
    REF_TRY(upload(c, &c->scales, in->scales, P * 3));
    REF_TRY(upload(c, &c->rotations, in->rotations, P * 4));
    REF_TRY(upload(c, &c->cov3D, in->cov3D_precomp, P * 6));
    REF_TRY(upload(c, &c->view, in->view, 16));
    REF_TRY(upload(c, &c->proj, in->proj, 16));
    REF_TRY(upload(c, &c->campos, in->campos, 3));
    REF_TRY(dev_alloc(c, (void**)&c->out_color, 3 * N * sizeof(float)));
    REF_TRY(dev_alloc(c, (void**)&c->out_depth, N * sizeof(float)));
    REF_TRY(dev_alloc(c, (void**)&c->radii, P * sizeof(int)));

    int R = -1;
    try {
        R = CudaRasterizer::Rasterizer::forward(
            chunk_allocator(c, &c->geom), chunk_allocator(c, &c->binning), chunk_allocator(c, &c->img),
            c->P, c->D, c->M, c->bg, c->W, c->H, c->means3D, c->shs, c->colors, c->opacities, c->scales,
            c->scale_modifier, c->rotations, c->cov3D, c->view, c->proj, c->campos, c->tan_fovx, c->tan_fovy,
            /*prefiltered=*/false, c->out_color, c->out_depth, c->radii);
    } catch (...) {
        rc = c->alloc_err != hipSuccess ? (int)c->alloc_err : REF_E_THROWN;
        (void)hipDeviceSynchronize();
        release(c);
        return rc;
    }
    REF_TRY((int)hipDeviceSynchronize());
    REF_TRY((int)hipGetLastError());
    if (R < 0) {
        release(c);
        return REF_E_STATE;
    }
    c->R = R;
    out->num_rendered = R;

    char* p = c->geom.ptr;
    CudaRasterizer::GeometryState geom = CudaRasterizer::GeometryState::fromChunk(p, P);
    p = c->img.ptr;
    CudaRasterizer::ImageState img = CudaRasterizer::ImageState::fromChunk(p, N);
    const size_t tiles = (size_t)((in->W + 15) / 16) * ((in->H + 15) / 16);
    REF_TRY(download(out->out_color, c->out_color, 3 * N));
    REF_TRY(download(out->out_depth, c->out_depth, N));
    REF_TRY(download(out->radii, c->radii, P));
    REF_TRY(download(out->means2D, geom.means2D, P));
    REF_TRY(download(out->depths, geom.depths, P));
    REF_TRY(download(out->conic_opacity, geom.conic_opacity, P));
    REF_TRY(download(out->rgb, geom.rgb, P * 3));
    REF_TRY(download(out->clamped, geom.clamped, P * 3));
    REF_TRY(download(out->tiles_touched, geom.tiles_touched, P));
    REF_TRY(download(out->final_T, img.accum_alpha, N));
    REF_TRY(download(out->n_contrib, img.n_contrib, N));
    REF_TRY(download(out->ranges, img.ranges, tiles));
#undef REF_TRY
    *ctx_out = c;
    return 0;
}

// BinningState::point_list (the sorted Gaussian ids) of a completed forward: n must be its num_rendered.
int ref_point_list(void* ctx, int* dst, int n) {
    Ctx* c = (Ctx*)ctx;
    if (!c || c->R < 0) return REF_E_STATE;
    if (n != c->R || (n > 0 && !dst)) return REF_E_ARG;
    if (n == 0) return 0;
    char* p = c->binning.ptr;
    CudaRasterizer::BinningState b = CudaRasterizer::BinningState::fromChunk(p, (size_t)c->R);
    return download(dst, b.point_list, (size_t)n);
}

// The reference backward (always BACKWARD::renderFused, with grad_power = power) on a completed forward.
int ref_backward(void* ctx, const float* dL_dpix, int power, RefGrads* out) {
    Ctx* c = (Ctx*)ctx;
    if (!c || c->R < 0 || !c->geom.ptr || !c->binning.ptr || !c->img.ptr) return REF_E_STATE;
    if (!dL_dpix || !out || power < 1) return REF_E_ARG;
    const size_t P = c->P, N = (size_t)c->W * c->H, M = c->M;
    // every gradient buffer of this call lives in one scope and is freed before returning
    Ctx* g = new Ctx;
    float *dpix = nullptr, *dmeans2D = nullptr, *dconic = nullptr, *dopacity = nullptr, *dcolors = nullptr,
          *dmeans3D = nullptr, *dcov3D = nullptr, *dsh = nullptr, *dscales = nullptr, *drot = nullptr;
    int rc = 0;
#define REF_TRY(expr)             \
    if ((rc = (expr)) != 0) {     \
        (void)hipDeviceSynchronize(); \
        release(g);               \
        return rc;                \
    }
    REF_TRY(upload(g, &dpix, dL_dpix, 3 * N));
    REF_TRY(dev_alloc(g, (void**)&dmeans2D, P * 3 * sizeof(float)));
    REF_TRY(dev_alloc(g, (void**)&dconic, P * 4 * sizeof(float)));
    REF_TRY(dev_alloc(g, (void**)&dopacity, P * sizeof(float)));
    REF_TRY(dev_alloc(g, (void**)&dcolors, P * 3 * sizeof(float)));
    REF_TRY(dev_alloc(g, (void**)&dmeans3D, P * 3 * sizeof(float)));
    REF_TRY(dev_alloc(g, (void**)&dcov3D, P * 6 * sizeof(float)));
    REF_TRY(dev_alloc(g, (void**)&dsh, P * M * 3 * sizeof(float)));
    REF_TRY(dev_alloc(g, (void**)&dscales, P * 3 * sizeof(float)));
    REF_TRY(dev_alloc(g, (void**)&drot, P * 4 * sizeof(float)));
    try {
        CudaRasterizer::Rasterizer::backward(
            c->P, c->D, c->M, c->R, c->bg, c->W, c->H, c->means3D, c->shs, c->colors, c->scales, c->scale_modifier,
            c->rotations, c->cov3D, c->view, c->proj, c->campos, c->tan_fovx, c->tan_fovy, c->radii, c->geom.ptr,
            c->binning.ptr, c->img.ptr, dpix, dmeans2D, dconic, dopacity, dcolors, dmeans3D, dcov3D, dsh, dscales,
            drot, power);
    } catch (...) {
        (void)hipDeviceSynchronize();
        release(g);
        return REF_E_THROWN;
    }
    REF_TRY((int)hipDeviceSynchronize());
    REF_TRY((int)hipGetLastError());
    REF_TRY(download(out->dmeans2D, dmeans2D, P * 3));
    REF_TRY(download(out->dcolors, dcolors, P * 3));
    REF_TRY(download(out->dopacity, dopacity, P));
    REF_TRY(download(out->dmeans3D, dmeans3D, P * 3));
    REF_TRY(download(out->dcov3D, dcov3D, P * 6));
    REF_TRY(download(out->dsh, dsh, P * M * 3));
    REF_TRY(download(out->dscales, dscales, P * 3));
    REF_TRY(download(out->drot, drot, P * 4));
#undef REF_TRY
    release(g);
    return 0;
}

// Rasterizer::markVisible: present[i] = 1 where the reference's frustum test keeps Gaussian i.
int ref_mark_visible(int P, const float* means3D, const float* view, const float* proj, unsigned char* present) {
    if (P <= 0 || P > (1 << 24) || !means3D || !view || !proj || !present) return REF_E_ARG;
    Ctx* g = new Ctx;
    float *m = nullptr, *v = nullptr, *pr = nullptr;
    bool* out = nullptr;
    int rc = 0;
#define REF_TRY(expr)             \
    if ((rc = (expr)) != 0) {     \
        (void)hipDeviceSynchronize(); \
        release(g);               \
        return rc;                \
    }
    REF_TRY(upload(g, &m, means3D, (size_t)P * 3));
    REF_TRY(upload(g, &v, view, 16));
    REF_TRY(upload(g, &pr, proj, 16));
    REF_TRY(dev_alloc(g, (void**)&out, (size_t)P * sizeof(bool)));
    CudaRasterizer::Rasterizer::markVisible(P, m, v, pr, out);
    REF_TRY((int)hipDeviceSynchronize());
    REF_TRY((int)hipGetLastError());
    static_assert(sizeof(bool) == 1, "present is copied out as bytes");
    REF_TRY(download(present, out, (size_t)P));
#undef REF_TRY
    release(g);
    return 0;
}

}  // extern "C"
