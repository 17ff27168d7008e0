// mi_rast.hip -- C-ABI implementation of include/mi_rast.h and host orchestration of the gfx950 rasterizer kernels (every other public
// header include/mi_X.h is implemented by the csrc/mi_X.hip of its name, and by that file alone).  Build: one object per .hip file,
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -munsafe-fp-atomics -fPIC (see seganygaussians_amd/build.py).  No torch, no pybind.
#include "host.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

// the binning stages in launch order: count (full or lean lists) -> range scan -> emit (full or lean) -> per-tile sort
#include "bin_full.h"
#include "bin_lean.h"
#include "tile_ranges.h"
#include "tile_sort.h"
#include "blend_bwd.h"
#include "blend_bwd_wave.h"   // (the profiling build compiles the PRODUCT kernel too: what tools/ measure is what ships; the ablation
                              // masks and rejected variants of rounds 2-5 are a record under tools/experiments/, compiled nowhere)
#include "blend_bwd_feat.h"   // features-only backward (MI_RAST_BWD_FEATURES_ONLY): one wave per half tile
#include "blend_fwd.h"
#include "blend_fwd_wave.h"
#ifdef MI_RAST_PROFILING
#include "blend_fwd_x3.h"   // round 2's tile-batched bf16x3 forward: A/B comparisons only (MI_RAST_TILE_FWD)
#endif
#include "common.h"
#include "fingerprint.h"
#include "geometry.h"
#include "lift.h"             // 2D-to-3D score lifting (mi_rast_lift): one front-to-back walk, one wave per half tile
#include "xcd_runs.h"
#include "xcd_stamp.h"        // (the profiling build's g_xcd_log is defined in this translation unit alone)

using namespace mirast;

namespace {

// Mirrors CHECK_CUDA (CF/cuda_rasterizer/auxiliary.h:166-173): with debug set, synchronise after each
// stage and surface the error; without it only launch errors are caught.  (c: the Call below.)
#define STAGE_CHECK(c, name)                                                                           \
    do {                                                                                               \
        hipError_t _e = hipGetLastError();                                                             \
        if (_e == hipSuccess && (c).debug) _e = hipStreamSynchronize((c).stream);                      \
        if (_e != hipSuccess)                                                                          \
            return fail(MI_RAST_ERR_HIP, std::string("[HIP ERROR] in stage ") + name + ": " + hipGetErrorString(_e)); \
    } while (0)

// ---- host-side scratch for the num_rendered read-back: pinned words + two events per (host thread, device) ----
constexpr int MAX_DEVICES = 64;
struct HostSync {
    int* pinned = nullptr;   // R partial sums, then {R, longest tile list} of the range scan
    int* pinned_dev = nullptr;  // the same buffer as the kernels address it (they store into it directly)
    uint64_t* fp = nullptr;     // partial fingerprints (mi_rast_fingerprint), [MI_FP_MAX][FP_BLOCKS]
    uint64_t* fp_dev = nullptr;
    hipEvent_t ev = nullptr;
    hipEvent_t ev2 = nullptr;
    bool ok = false;
    // the words behind the R partial sums (tile_ranges.h: NR_*), as the host reads them and as the range scan addresses them
    const int* words() const { return pinned + R_SLOTS * R_SLOT_STRIDE; }
    int* words_dev() const { return pinned_dev + R_SLOTS * R_SLOT_STRIDE; }
    bool init()
    {
        if (ok) return true;
        if (hipHostMalloc((void**)&pinned, (R_SLOTS * R_SLOT_STRIDE + 16) * sizeof(int), hipHostMallocMapped) != hipSuccess) return false;
        if (hipHostGetDevicePointer((void**)&pinned_dev, pinned, 0) != hipSuccess) return false;
        if (hipHostMalloc((void**)&fp, (size_t)MI_FP_MAX * FP_BLOCKS * sizeof(uint64_t), hipHostMallocMapped) != hipSuccess) return false;
        if (hipHostGetDevicePointer((void**)&fp_dev, fp, 0) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&ev2, hipEventDisableTiming) != hipSuccess) return false;
        ok = true;
        return true;
    }
    // (a host thread's scratch goes with the thread; errors are ignored: at process exit the runtime may be gone already)
    ~HostSync()
    {
        if (ev) (void)hipEventDestroy(ev);
        if (ev2) (void)hipEventDestroy(ev2);
        if (pinned) (void)hipHostFree(pinned);
        if (fp) (void)hipHostFree(fp);
    }
};
thread_local HostSync g_host_sync_tl[MAX_DEVICES];
thread_local int g_last_longest_run[MAX_DEVICES];   // of this thread's last forward per device (mi_rast_last_longest_run)

int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return -1;
    return dev;
}

// ---- per-stage profiling (bench.py) -----------------------------------------------------------
// A measurement aid, not part of the rendering state: one process-wide switch, one event set per device (created on
// first use on that device).  Toggle only while no call is in flight (include/mi_rast.h).
std::atomic<bool> g_profile{false};
struct ProfileEvents {
    hipEvent_t ev[MI_STAGE_COUNT][2];
    std::atomic<bool> created{false};   // read outside the mutex while another host thread's forward may be creating the events
    bool used[MI_STAGE_COUNT] = {};
};
ProfileEvents g_prof[MAX_DEVICES];
std::mutex g_prof_mutex;

ProfileEvents* profile_events(int dev)
{
    if (dev < 0) return nullptr;
    ProfileEvents& pe = g_prof[dev];
    if (!pe.created.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lock(g_prof_mutex);
        if (!pe.created.load(std::memory_order_relaxed)) {
            for (int i = 0; i < MI_STAGE_COUNT; i++)
                for (int k = 0; k < 2; k++)
                    if (hipEventCreate(&pe.ev[i][k]) != hipSuccess) return nullptr;
            pe.created.store(true, std::memory_order_release);
        }
    }
    return &pe;
}

struct StageTimer {
    hipStream_t s;
    int stage;
    ProfileEvents* pe;
    StageTimer(hipStream_t s_, int stage_) : s(s_), stage(stage_), pe(nullptr)
    {
        if (g_profile.load(std::memory_order_relaxed)) pe = profile_events(current_device());
        if (pe) (void)hipEventRecord(pe->ev[stage][0], s);
    }
    ~StageTimer()
    {
        if (pe) {
            (void)hipEventRecord(pe->ev[stage][1], s);
            pe->used[stage] = true;
        }
    }
};

ViewParams make_view(const float* view_d, const float* proj_d, const float* campos_d, float tan_fovx, float tan_fovy,
                     float scale_modifier, int W, int H)
{
    ViewParams vp;
    vp.view = view_d;
    vp.proj = proj_d;
    vp.campos = campos_d;
    vp.tan_fovx = tan_fovx;
    vp.tan_fovy = tan_fovy;
    // CF/cuda_rasterizer/rasterizer_impl.cu:222-223
    vp.focal_y = H / (2.0f * tan_fovy);
    vp.focal_x = W / (2.0f * tan_fovx);
    vp.scale_modifier = scale_modifier;
    vp.W = W;
    vp.H = H;
    vp.grid_x = (W + TILE_X - 1) / TILE_X;
    vp.grid_y = (H + TILE_Y - 1) / TILE_Y;
    return vp;
}
// the view of a call that only blends over the buffers a forward left: the image size and the tile grid, everything else zero
ViewParams make_blend_view(int W, int H)
{
    ViewParams vp;
    std::memset(&vp, 0, sizeof(vp));
    vp.W = W;
    vp.H = H;
    vp.grid_x = (W + TILE_X - 1) / TILE_X;
    vp.grid_y = (H + TILE_Y - 1) / TILE_Y;
    return vp;
}

struct GeomPtrs {
    float* depths;
    float2* means2D;
    float4* conic_opacity;
    float* cov3D;
    float* rgb;
    uint8_t* clamped;
    uint32_t* tiles_touched;
    uint32_t* depth_key;
    BlendRec* index_rec;  // [P] {mean, id, radius, conic + opacity} in index order (written by the preprocess pass for visible Gaussians)
    int* cull_counter;    // one word: Gaussians culled although `prefiltered` was set
    unsigned long long* band_bits;  // [MAX_BANDS][ceil(P / 64)]: per band of tile rows, one bit per Gaussian whose rect reaches it (bin_lean.h)
    float* bwd_pack;  // [P,8] packed per-Gaussian field gradients (backward scratch)
};
struct ImgPtrs {
    float* final_T;
    uint32_t* n_contrib;
    uint2* ranges;
    uint32_t* tile_consumed;  // per tile: list entries the forward blend consumed (counter E of SURVEY.md 8d)
    uint32_t* tile_count;
    uint32_t* tile_cursor;
    int* num_rendered;
    uint32_t* tile_nsurv;   // per tile: blend-list entries the forward walked
    uint32_t* run_bounds;   // [9]: the blend kernels' XCD runs of tiles (xcd_runs.h: XcdRuns): from the range scan (equal counts, or equal
                            // modelled work)
    int* words() const { return num_rendered + R_SLOTS * R_SLOT_STRIDE; }   // the words behind the R partial sums (tile_ranges.h: NR_*)
};
struct BinPtrs {
    uint2* entries;      // per overlap: {depth bits, Gaussian id | quadrant mask << 28}, bucketed by tile (unsorted inside a tile)
    uint2* scratch;      // ping-pong buffer for tiles too long for the LDS sort
    uint32_t* blend_list;  // per tile at range.x, in depth order: Gaussian id | quadrant mask << 28 (tile_sort.h: emit_blend_list); full
                           // lists: the low 28 bits are the reference's point_list
};

GeomPtrs geom_from(char* base, int P)
{
    size_t off[MI_GEOM_NFIELDS];
    mi_rast_geometry_layout(P, off);
    GeomPtrs g;
    g.depths = (float*)(base + off[MI_GEOM_DEPTHS]);
    g.means2D = (float2*)(base + off[MI_GEOM_MEANS2D]);
    g.conic_opacity = (float4*)(base + off[MI_GEOM_CONIC_OPACITY]);
    g.cov3D = (float*)(base + off[MI_GEOM_COV3D]);
    g.rgb = (float*)(base + off[MI_GEOM_RGB]);
    g.clamped = (uint8_t*)(base + off[MI_GEOM_CLAMPED]);
    g.tiles_touched = (uint32_t*)(base + off[MI_GEOM_TILES_TOUCHED]);
    g.depth_key = (uint32_t*)(base + off[MI_GEOM_DEPTH_KEY]);
    g.index_rec = (BlendRec*)(base + off[MI_GEOM_INDEX_REC]);
    g.cull_counter = (int*)(base + off[MI_GEOM_CULL_COUNTER]);
    g.band_bits = (unsigned long long*)(base + off[MI_GEOM_BAND_BITS]);
    g.bwd_pack = (float*)(base + off[MI_GEOM_BWD_PACK]);
    return g;
}
ImgPtrs img_from(char* base, int W, int H)
{
    size_t off[MI_IMG_NFIELDS];
    mi_rast_image_layout(W, H, off);
    ImgPtrs m;
    m.final_T = (float*)(base + off[MI_IMG_FINAL_T]);
    m.n_contrib = (uint32_t*)(base + off[MI_IMG_N_CONTRIB]);
    m.ranges = (uint2*)(base + off[MI_IMG_RANGES]);
    m.tile_consumed = (uint32_t*)(base + off[MI_IMG_TILE_CONSUMED]);
    m.tile_count = (uint32_t*)(base + off[MI_IMG_TILE_COUNT]);
    m.tile_cursor = (uint32_t*)(base + off[MI_IMG_TILE_CURSOR]);
    m.num_rendered = (int*)(base + off[MI_IMG_NUM_RENDERED]);
    m.tile_nsurv = (uint32_t*)(base + off[MI_IMG_TILE_NSURV]);
    m.run_bounds = reinterpret_cast<uint32_t*>(m.words() + NR_RUN_BOUNDS);
    return m;
}
BinPtrs bin_from(char* base, int R)
{
    size_t off[MI_BIN_NFIELDS];
    mi_rast_binning_layout(R, off);
    BinPtrs b;
    b.entries = (uint2*)(base + off[MI_BIN_ENTRIES]);
    b.scratch = (uint2*)(base + off[MI_BIN_SCRATCH]);
    b.blend_list = (uint32_t*)(base + off[MI_BIN_BLEND_LIST]);
    return b;
}

// RGB (+ the DEPTH variant's mask / depth planes), or a feature of any width from 1 to MAX_CHANNELS (the reference compiles ANY ONE
// NUM_CHANNELS into its kernels, CF/cuda_rasterizer/config_contrastive_f.h:15): blended in channel blocks of 64 / 32 / 16, the last one
// possibly PARTIAL -- fewer real channels, zeros in the MFMA operands behind them, as RGB has always been rendered (3 of 16).  Every
// pass re-evaluates alpha and T; the contraction over channels is linear, so the backward's per-block geometry gradients add up in the
// packed record.
constexpr int MAX_CHANNELS = 256;
constexpr int MAX_CHANNEL_BLOCKS = MAX_CHANNELS / 16;
// bytes of the geometry buffer's bwd_pack field: the packed per-Gaussian field gradients + the backward's work-queue counters (one set
// of eight per channel block); zero when mi_rast_backward starts its blend pass
inline size_t bwd_pack_bytes(int P)
{
    return (size_t)(P > 0 ? P : 1) * 8 * sizeof(float) + MAX_CHANNEL_BLOCKS * 8 * XCD_QUEUE_STRIDE * sizeof(uint32_t);
}
bool channels_supported(int c) { return c >= 1 && c <= MAX_CHANNELS; }
// One launch's share of a feature: channels [c0, c0 + real), blended by the kernel instantiation for `width` channels (real < width: PARTIAL)
struct ChannelBlock { int c0, width, real; };
// The one plan of all three blend passes: calls f(block) for the blocks of a `channels`-wide feature in order -- 64 channels while
// that many are left, then halving down to `smallest`; what is left behind the last whole block is one partial block of `smallest`
// (the forward: 32, 1 .. 31 channels of it real; the backwards and the profiling build's comparison forwards: 16).
template <class F>
void for_channel_blocks(int channels, int smallest, F&& f)
{
    for (int c0 = 0, width = 64; c0 < channels; c0 += width) {
        while (width > smallest && channels - c0 < width) width >>= 1;
        f(ChannelBlock{c0, width, std::min(width, channels - c0)});
    }
}

// Run-time value -> compile-time constant: each calls the generic lambda f with a std::integral_constant whose ::value names the
// kernel instantiation.  An arm no caller takes is closed with `if constexpr` inside f, so that it instantiates no kernel.
template <class F>
void with_bool(bool b, F&& f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
void with_bools(bool a, bool b, F&& f)
{
    with_bool(a, [&](auto ka) { with_bool(b, [&](auto kb) { f(ka, kb); }); });
}
template <class F>
void with_exp_mode(int xm, F&& f)   // common.h: ExpMode
{
    if (xm == EXP_HYBRID) f(std::integral_constant<int, EXP_HYBRID>{});
    else if (xm == EXP_EXACT) f(std::integral_constant<int, EXP_EXACT>{});
    else f(std::integral_constant<int, EXP_FAST>{});
}

// what mi_rast_forward and mi_rast_forward_reuse refuse alike
int check_forward_args(int P, int channels, int width, int height, const float* colors_precomp, const float* mask)
{
    if (P <= 0 || width <= 0 || height <= 0) return fail(MI_RAST_ERR_INVALID, "P, width and height must be positive");
    if (!channels_supported(channels)) return fail(MI_RAST_ERR_INVALID, "unsupported channel count (supported: 1 .. 256)");
    if (mask && channels != 3) return fail(MI_RAST_ERR_INVALID, "mask/depth variant is built for 3 channels");
    // CF/cuda_rasterizer/rasterizer_impl.cu:242-245
    if (channels != 3 && colors_precomp == nullptr)
        return fail(MI_RAST_ERR_NON_RGB, "For non-RGB, provide precomputed Gaussian colors!");
    return MI_RAST_OK;
}

// How the blend kernels' tiles are dealt to the eight XCDs (xcd_runs.h, blend_fwd_wave.h: fwd_wave_item, tile_ranges.h: tile_ranges_kernel):
// one run of tiles per XCD, both blend kernels, boundaries from the range scan.
// Measured in round 5 (profiles/r05_xcd_balance.md; cfg3s = density varying over the image, cfg3 = uniform): equal tile counts 447 / 844
// views/s; this model 493 / 835 (cap 384 ... 1024, fix 32 ... 128 tried: 768 / 128 best; no cap -- the list length -- 428: a long list
// on an opaque surface is a SHORT walk); m = 4 interleaved equal-count runs in the forward + the walk scan for the backward 497 / 831.
// (Both of those were removed later; so was cutting the backward's runs at what the forward really walked, measured in round 6 at
// 530.2 / 529.1 / 530.8 views/s for never / when the density varies / always -- DESIGN.md section 11.)
constexpr int RUN_MODEL_CAP = 768;    // range scan: XCD runs of equal sum(min(list length, cap) + fix); 0: equal tile counts
constexpr int RUN_MODEL_FIX = 128;    // a tile's fixed cost (four waves' start-up) in list entries
inline uint32_t longest_of(const int* bounds, uint32_t ntiles)
{
    uint32_t longest = 0;
    for (int x = 0; x < 8; x++) {
        const uint32_t a = (uint32_t)bounds[x], b = (uint32_t)bounds[x + 1];
        longest = std::max(longest, b >= a ? b - a : 0u);
    }
    return std::min(std::max(longest, (ntiles + 7u) >> 3), xcd_max_run(ntiles));
}

// What the stage and launch functions of one call share: the view, the stream, the caller's switches, the fields of the three buffers.
struct Call {
    ViewParams vp;
    hipStream_t stream;
    int debug, flags, P;
    GeomPtrs geom;
    ImgPtrs img;
    BinPtrs bin;
    uint32_t longest_run;   // of the XCD runs of tiles (a forward reads it at the ev2 wait, a reuse is handed it; 0: unknown): the forward blend's grid
    uint32_t ntiles() const { return vp.grid_x * vp.grid_y; }
    size_t HW() const { return (size_t)vp.W * vp.H; }   // floats of one image plane
    bool antialias() const { return (flags & MI_RAST_ANTIALIAS) != 0; }   // the two geometry kernels: antialias.h
    bool xexp() const { return (flags & MI_RAST_FAST_EXP) == 0; }   // the device library's expf (common.h gauss_exp), the default
    // the wave-per-quadrant forward kernels: common.h ExpMode
    int exp_mode() const { return (flags & MI_RAST_FAST_EXP) ? EXP_FAST : (flags & MI_RAST_EXACT_EXP) ? EXP_EXACT : EXP_HYBRID; }
};

// What the caller of mi_rast_forward / mi_rast_mask_forward hands to the stages before the blend
struct FrontArgs {
    mi_rast_resize_fn geometry_buffer, binning_buffer, image_buffer;
    void *geometry_user, *binning_user, *image_user;
    int D, M, colors_given, prefiltered;
    const float *means3D, *shs, *opacities, *scales, *rotations, *cov3D_precomp;
    int* radii;
};

// How the count and emit passes walk the tile grid (bin_full.h, bin_lean.h)
struct BinPlan {
    // FULL lists (parity tests): images with more tiles than one launch of the full count / emit passes has LDS counters for are walked
    // in bands of tile rows by the host (grid_x + 2: the count pass keeps band_rows (+ 1) rows of an odd stride >= grid_x + 1)
    uint32_t band_rows, nbands;
    // LEAN lists: <= MAX_BANDS device-side bands of lean_band_h tile rows, every workgroup of the count / emit passes in one of them
    uint32_t lean_band_h, lean_nbands;
    // Full lists (the reference's point_list and full-list positions) are materialised on request -- the reference's
    // `debug` flag or MI_RAST_FULL_LISTS -- ; otherwise only the overlaps that pass the cull are listed.
    bool nocull, full;
    // full lists: <= 256 workgroups of 1024 threads, each a slice of the Gaussians (64-index chunks dealt round robin); lean lists:
    // workgroups dealt to the bands in proportion to the bands' Gaussian counts (bin_lean.h: band_plan), at least one per band
    int nwg;
};
// (refuses what the passes cannot index, before any buffer is asked for or any work queued)
int plan_binning(const Call& c, BinPlan& bp)
{
    const ViewParams& vp = c.vp;
    if (c.P >= (1 << ID_BITS)) return fail(MI_RAST_ERR_INVALID, "more than 2^28 Gaussians");
    if (vp.grid_x > 1023u || vp.grid_y > 2047u)
        return fail(MI_RAST_ERR_INVALID, "image too large: more than 1023 tiles across or 2047 tiles down");
    bp.band_rows = std::min<uint32_t>(vp.grid_y, std::max<uint32_t>(1u, (uint32_t)BIN_MAX_TILES / (vp.grid_x + 2u) - 1u));
    bp.nbands = (vp.grid_y + bp.band_rows - 1) / bp.band_rows;
    bp.lean_band_h = bp.lean_nbands = 1;
    if (!band_geometry(vp.grid_x, vp.grid_y, SPAN_MAX_HEAD_WORDS, bp.lean_band_h, bp.lean_nbands))
        return fail(MI_RAST_ERR_INVALID, "image too large for the banded binning passes (more than 24 bands of tile rows at this width)");
    bp.nocull = (c.flags & MI_RAST_NO_CULL) != 0;
    bp.full = c.debug != 0 || bp.nocull || (c.flags & MI_RAST_FULL_LISTS) != 0;
    bp.nwg = bp.full ? bin_workgroups(c.P) : std::min(BIN_LEAN_WG, (int)bp.lean_nbands + (c.P + 1023) / 1024);
    return MI_RAST_OK;
}

int preprocess_stage(const Call& c, const FrontArgs& a, const BinPlan& bp)
{
    const int P = c.P, ntiles = (int)c.ntiles();
    if (a.prefiltered) HIP_TRY(hipMemsetAsync(c.geom.cull_counter, 0, sizeof(int), c.stream));
    {
        StageTimer t(c.stream, MI_STAGE_PREPROCESS);
        HIP_TRY(hipMemsetAsync(c.img.num_rendered, 0, R_SLOTS * R_SLOT_STRIDE * sizeof(int), c.stream));
        // (the per-tile entry totals are zeroed by the preprocess kernel's first threads; fewer Gaussians than tiles: by a fill)
        if (P < ntiles) HIP_TRY(hipMemsetAsync(c.img.tile_cursor, 0, (size_t)ntiles * sizeof(uint32_t), c.stream));
        // SH colours: the workgroup's coefficient rows are staged in LDS (geometry.h), 256 rows of 3 M + 4 floats
        const size_t sh_lds = a.colors_given ? 0 : (size_t)256 * (3 * (size_t)a.M + 4) * sizeof(float);
        if (sh_lds > 64 * 1024) return fail(MI_RAST_ERR_INVALID, "too many SH coefficients per Gaussian (at most 16: degree 3)");
        with_bool(c.antialias(), [&](auto aa) {
            hipLaunchKernelGGL(preprocess_fwd_kernel<decltype(aa)::value>, dim3((P + 255) / 256), dim3(256), sh_lds, c.stream, P, a.D, a.M, a.means3D,
                               a.scales, a.rotations, a.opacities, a.shs, c.geom.clamped, a.cov3D_precomp, a.colors_given, c.vp, a.radii,
                               c.geom.means2D, c.geom.depths, c.geom.cov3D, c.geom.rgb, c.geom.conic_opacity, c.geom.tiles_touched,
                               c.geom.depth_key, c.geom.index_rec, c.img.num_rendered, a.prefiltered, c.geom.cull_counter,
                               c.geom.band_bits, bp.lean_band_h, bp.lean_nbands, c.img.tile_cursor, (uint32_t)ntiles);
        });
    }
    STAGE_CHECK(c, "preprocess");
    if (a.prefiltered) {
        int culled = 0;
        HIP_TRY(hipMemcpyAsync(&culled, c.geom.cull_counter, sizeof(int), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        if (culled)
            return fail(MI_RAST_ERR_INVALID, "Point is filtered although prefiltered is set. This shouldn't happen!");
    }
    return MI_RAST_OK;
}

// One-time opt-in to > 64 KB of dynamic LDS (gfx950: 160 KB per workgroup), per device.
std::atomic<bool> g_attr_set[MAX_DEVICES];
std::mutex g_attr_mutex;
int opt_in_to_large_lds(int dev)
{
    if (g_attr_set[dev].load(std::memory_order_acquire)) return MI_RAST_OK;
    std::lock_guard<std::mutex> lock(g_attr_mutex);
    if (g_attr_set[dev].load(std::memory_order_relaxed)) return MI_RAST_OK;
    const int max_lds = (int)((BIN_MAX_TILES + 11 * 1024 + 16) * sizeof(uint32_t));
    HIP_TRY(hipFuncSetAttribute((const void*)bin_ranks_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    HIP_TRY(hipFuncSetAttribute((const void*)bin_ranks_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    HIP_TRY(hipFuncSetAttribute((const void*)bin_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
    // (160 KB per workgroup less the kernels' static words: the band plan)
    HIP_TRY(hipFuncSetAttribute((const void*)bin_spans_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    HIP_TRY(hipFuncSetAttribute((const void*)bin_spans_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    HIP_TRY(hipFuncSetAttribute((const void*)tile_ranges_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (BIN_MAX_TILES_TOTAL + 1) * (int)sizeof(uint32_t)));
    g_attr_set[dev].store(true, std::memory_order_release);
    return MI_RAST_OK;
}

// count pass over slices, scan over (tile, slice), scan over tiles -> ranges (bin_full.h, tile_ranges.h; lean lists: bin_lean.h).  R is known after the preprocess pass; the
// count pass stores its partial sums into the host's pinned buffer (event ev), and the host reads them while the scans run.
int count_and_scan_stage(const Call& c, const BinPlan& bp, const HostSync& hs)
{
    const int P = c.P, ntiles = (int)c.ntiles();
    {
        StageTimer t(c.stream, MI_STAGE_TILE_SCAN);
        if (bp.full) {
            const size_t cnt_lds = (size_t)(bp.band_rows + 1) * count_grid_stride(c.vp.grid_x) * sizeof(int);
            for (uint32_t b = 0; b < bp.nbands; b++) {
                const uint32_t by0 = b * bp.band_rows, by1 = std::min(c.vp.grid_y, by0 + bp.band_rows);
                hipLaunchKernelGGL(bin_count_kernel, dim3(bp.nwg), dim3(BIN_THREADS), cnt_lds, c.stream, P, c.geom.index_rec, c.geom.depth_key,
                                   c.img.tile_count, c.vp.grid_x, c.vp.grid_y, by0, by1, (const int*)c.img.num_rendered,
                                   b == 0 ? hs.pinned_dev : (int*)nullptr);
            }
        } else {
            hipLaunchKernelGGL(bin_spans_kernel<false>, dim3(bp.nwg), dim3(1024),
                               span_lds_bytes((size_t)bp.lean_band_h * count_grid_stride(c.vp.grid_x)), c.stream, P, c.geom.index_rec,
                               c.geom.depth_key, c.geom.band_bits, c.img.tile_count, c.img.tile_cursor, (const uint2*)nullptr, (uint2*)nullptr,
                               c.vp.grid_x, c.vp.grid_y, bp.lean_band_h, bp.lean_nbands, (const int*)c.img.num_rendered, hs.pinned_dev);
        }
        HIP_TRY(hipEventRecord(hs.ev, c.stream));
        // (one launch for both scans -- every workgroup scans its tiles over the slices, the last one to finish scans the totals
        // behind a device-scope counter and agent-scope fences -- was built and measured in round 4: tile scan 0.058 -> 0.060 ms
        // on cfg3; the fences and the serial tail inside the kernel cost more than the launch they save)
        // full lists: scan over (tile, slice); lean lists: the count pass left the tile totals and every workgroup's offset itself
        if (bp.full)
            hipLaunchKernelGGL(scan_partials_kernel, dim3((ntiles + 63) / 64), dim3(1024), 0, c.stream, ntiles, bp.nwg,
                               c.img.tile_count, c.img.tile_cursor);
        const uint32_t run_cap = !(c.flags & MI_RAST_EQUAL_RUNS) ? (uint32_t)RUN_MODEL_CAP : 0u;
        hipLaunchKernelGGL(tile_ranges_kernel, dim3(1), dim3(1024),
                           ((size_t)std::min(ntiles, BIN_MAX_TILES_TOTAL) + 1) * sizeof(uint32_t), c.stream, ntiles, c.img.tile_cursor,
                           c.img.ranges, c.img.words(), (const int*)c.img.num_rendered, hs.words_dev(), c.img.tile_consumed, c.img.tile_nsurv,
                           c.img.run_bounds, run_cap, (uint32_t)RUN_MODEL_FIX);
    }
    STAGE_CHECK(c, "tile scan");
    return MI_RAST_OK;
}

// The emit pass: every overlap into its tile's bucket of bin.entries, unsorted (bin_full.h, bin_lean.h)
int emit_stage(const Call& c, const BinPlan& bp, int R)
{
    const int P = c.P, ntiles = (int)c.ntiles();
    const bool verify = !bp.full && (c.flags & MI_RAST_VERIFY_LISTS) != 0;
    if (verify) HIP_TRY(hipMemsetAsync(c.bin.entries, 0, (size_t)R * sizeof(uint2), c.stream));
    {
        StageTimer t(c.stream, MI_STAGE_EMIT);
        if (bp.full) {
            const size_t band_tiles = (size_t)bp.band_rows * c.vp.grid_x;
            const size_t emit_lds = ((size_t)((band_tiles + 3) & ~(size_t)3) + 11 * 1024 + 16) * sizeof(uint32_t);
            for (uint32_t b = 0; b < bp.nbands; b++) {
                const uint32_t by0 = b * bp.band_rows, by1 = std::min(c.vp.grid_y, by0 + bp.band_rows);
                with_bool(bp.nocull, [&](auto nocull) {
                    hipLaunchKernelGGL(bin_ranks_kernel<decltype(nocull)::value>, dim3(bp.nwg), dim3(BIN_THREADS), emit_lds, c.stream, P, c.geom.index_rec,
                                       c.geom.depth_key, c.img.tile_count, c.img.ranges, c.bin.entries, c.vp.grid_x, c.vp.grid_y, by0, by1);
                });
            }
        } else {
            hipLaunchKernelGGL(bin_spans_kernel<true>, dim3(bp.nwg), dim3(1024), span_lds_bytes((size_t)bp.lean_band_h * c.vp.grid_x), c.stream,
                               P, c.geom.index_rec, c.geom.depth_key, c.geom.band_bits, c.img.tile_count, c.img.tile_cursor, c.img.ranges, c.bin.entries,
                               c.vp.grid_x, c.vp.grid_y, bp.lean_band_h, bp.lean_nbands, (const int*)c.img.num_rendered, (int*)nullptr);
        }
    }
    STAGE_CHECK(c, "emit entries");
    if (verify) {   // debugging aid: synchronous
        uint32_t* ctr = reinterpret_cast<uint32_t*>(c.img.words() + NR_VERIFY);
        HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(uint32_t), c.stream));
        hipLaunchKernelGGL(verify_entries_kernel, dim3(ntiles), dim3(256), 0, c.stream, (uint32_t)ntiles, c.img.ranges, c.bin.entries, ctr);
        uint32_t unwritten = 0;
        HIP_TRY(hipMemcpyAsync(&unwritten, ctr, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        if (unwritten)
            return fail(MI_RAST_ERR_HIP, "internal error: " + std::to_string(unwritten) + " list slots were counted but not emitted "
                                         "(count / emit passes of bin_spans_kernel disagree)");
    }
    return MI_RAST_OK;
}

// The range scan stores {total, longest list, ..., run boundaries} into this thread's pinned words (event ev2): no forward returns
// while that store can still land (the next forward of this thread, on another stream, would read them).
int take_longest_run(Call& c, const HostSync& hs, int dev)
{
    HIP_TRY(hipEventSynchronize(hs.ev2));
    c.longest_run = longest_of(hs.words() + NR_RUN_BOUNDS, c.ntiles());
    g_last_longest_run[dev] = (int)c.longest_run;
    return MI_RAST_OK;
}

template <int CLASS>
void launch_tile_sort_wave(const Call& c)
{
    hipLaunchKernelGGL(tile_sort_wave_kernel<CLASS>, dim3((c.ntiles() + 3) / 4), dim3(256), 0, c.stream, c.ntiles(), c.img.ranges,
                       (const uint2*)c.bin.entries, c.bin.blend_list);
}
template <int LO, int CAP, bool FB, int NT>
void launch_tile_sort(const Call& c)
{
    hipLaunchKernelGGL((tile_sort_kernel<LO, CAP, FB, NT>), dim3(c.ntiles()), dim3(NT), 0, c.stream, c.ntiles(), c.img.ranges, c.bin.entries,
                       c.bin.scratch, (const int*)(c.img.words() + NR_KEY_BITS), c.bin.blend_list);
}

// lists of up to 4096 entries: one wave per tile (bitonic network in registers, three length classes); longer ones: two classes of the LDS radix
// sort (1024 threads + 112 KB, 1024 threads + 144 KB / HBM ping-pong), launched only if some tile needs them.  The longest
// list was copied to the host right after the range scan, which finished before the emit pass even started: this
// wait does not stall the queue.
int sort_stage(Call& c, const BinPlan& bp, const HostSync& hs, int dev, int R)
{
    {
        StageTimer t(c.stream, MI_STAGE_TILE_SORT);
        launch_tile_sort_wave<0>(c);
        if (int rc = take_longest_run(c, hs, dev)) return rc;
        // lean lists: the counts are the lists' exact lengths (bin_spans_kernel), their sum a lower bound of R
        if (bp.full ? hs.words()[NR_TOTAL] != R : hs.words()[NR_TOTAL] > R)
            return fail(MI_RAST_ERR_HIP, "internal error: tile counts do not add up to num_rendered");
        const int max_tile_count = hs.words()[NR_LONGEST];
        if (max_tile_count > 1024) launch_tile_sort_wave<1>(c);
        if (max_tile_count > 2048) launch_tile_sort_wave<2>(c);
        if (max_tile_count > TILE_SORT_WAVE_MAX) launch_tile_sort<TILE_SORT_WAVE_MAX, 6144, false, 1024>(c);
        if (max_tile_count > 6144) launch_tile_sort<6144, 8192, true, 1024>(c);
    }
    STAGE_CHECK(c, "tile sort");
    return MI_RAST_OK;
}

// Stages shared by forward and mask_forward: CF/cuda_rasterizer/rasterizer_impl.cu:246-317.
int geometry_and_binning(Call& c, const FrontArgs& a, int* num_rendered)
{
    const int dev = current_device();
    if (dev < 0) return fail(MI_RAST_ERR_HIP, "hipGetDevice failed (or device ordinal >= 64)");
    HostSync& hs = g_host_sync_tl[dev];
    BinPlan bp;
    if (int rc = plan_binning(c, bp)) return rc;
    size_t goff[MI_GEOM_NFIELDS], ioff[MI_IMG_NFIELDS], boff[MI_BIN_NFIELDS];
    char* geom_base = a.geometry_buffer(mi_rast_geometry_layout(c.P, goff), a.geometry_user);
    if (!geom_base) return fail(MI_RAST_ERR_ALLOC, "geometry buffer callback returned NULL");
    c.geom = geom_from(geom_base, c.P);
    char* img_base = a.image_buffer(mi_rast_image_layout(c.vp.W, c.vp.H, ioff), a.image_user);
    if (!img_base) return fail(MI_RAST_ERR_ALLOC, "image buffer callback returned NULL");
    c.img = img_from(img_base, c.vp.W, c.vp.H);

    if (int rc = preprocess_stage(c, a, bp)) return rc;
    if (int rc = opt_in_to_large_lds(dev)) return rc;
    if (!hs.init()) return fail(MI_RAST_ERR_HIP, "cannot allocate pinned host buffer / event");
    if (int rc = count_and_scan_stage(c, bp, hs)) return rc;
    HIP_TRY(hipEventRecord(hs.ev2, c.stream));
    // rasterizer_impl.cu:280-281: the host needs num_rendered to size the binning buffer.  We wait only for
    // the copy (event), not for the work queued behind it.
    HIP_TRY(hipEventSynchronize(hs.ev));
    long long Rsum = 0;
    for (int k = 0; k < R_SLOTS; k++) Rsum += hs.pinned[k * R_SLOT_STRIDE];
    if (Rsum > 0x7fffffffll) return fail(MI_RAST_ERR_INVALID, "more than 2^31 tile overlaps");
    const int R = (int)Rsum;
    *num_rendered = R;

    char* bin_base = a.binning_buffer(mi_rast_binning_layout(R, boff), a.binning_user);
    if (!bin_base) return fail(MI_RAST_ERR_ALLOC, "binning buffer callback returned NULL");
    c.bin = bin_from(bin_base, R);
    // no overlap at all: every tile's range is {0, 0}, and the blend kernels read no list
    if (R == 0) return take_longest_run(c, hs, dev);
    if (int rc = emit_stage(c, bp, R)) return rc;
    return sort_stage(c, bp, hs, dev, R);
}

// What a forward blends (features: `channels` per Gaussian; mask: the DEPTH variant's) and a backward blend pass reads and writes
struct FwdArgs { int channels; const float *features, *mask, *bg; float *out_color, *out_mask, *out_depth; };
struct BwdArgs { int channels; const float *bg, *colors, *dL_dpix, *dL_dout_mask; float* dL_dcolor; };

// The tile-batched kernel (blend_fwd.h): the mask-only forward; in the profiling build also a comparison kernel.  b: {0, C, C}, or one
// 64 / 32 / 16-channel block of a wider feature, of the last one possibly only b.real channels (blend_fwd.h PARTIAL)
template <int C, int EXTRA>
void launch_blend_fwd(const Call& c, const FwdArgs& a, ChannelBlock b)
{
    constexpr bool MAY_BE_PARTIAL = C == 16 && EXTRA == 0;
    with_bools(MAY_BE_PARTIAL && b.real < C, c.xexp(), [&](auto partial, auto xexp) {
        if constexpr (MAY_BE_PARTIAL || !decltype(partial)::value)
            hipLaunchKernelGGL((blend_fwd_kernel<C, EXTRA, decltype(xexp)::value, decltype(partial)::value>), dim3(c.vp.grid_x, c.vp.grid_y), dim3(256), 0,
                               c.stream, c.img.ranges, c.bin.blend_list, c.geom.index_rec, c.vp.W, c.vp.H, a.features + b.c0, a.mask, c.geom.depths,
                               c.img.final_T, c.img.n_contrib, c.img.tile_consumed, c.img.tile_nsurv, a.bg + b.c0,
                               a.out_color + b.c0 * c.HW(), a.out_mask, a.out_depth, a.channels, b.real);
    });
}

// One wave per (tile, quadrant): 32 x the longest XCD run of tiles workgroups (blend_fwd_wave.h).  The first launch of a forward takes
// the zero fill; the launches of further channel blocks fill nothing.
uint32_t fwd_wave_grid(const Call& c) { return 32u * (c.longest_run ? c.longest_run : xcd_max_run(c.ntiles())); }
// b: a 64- or 32-channel block; the remainder of a feature is a 32-channel block of which b.real channels exist (blend_fwd_wave.h PARTIAL)
template <int C>
void launch_blend_fwd_wave(const Call& c, const FwdArgs& a, ChannelBlock b, FwdZeroFill& zfill)
{
    const FwdZeroFill zf = std::exchange(zfill, FwdZeroFill{nullptr, 0u, nullptr, 0u});
    const bool is_partial = C == 32 && b.real < C;
    with_bools(is_partial, is_partial || a.channels != C, [&](auto partial, auto strided) {
        constexpr bool PARTIAL = decltype(partial)::value, STRIDED = decltype(strided)::value;
        with_exp_mode(c.exp_mode(), [&](auto xm) {
            if constexpr (!PARTIAL || (C == 32 && STRIDED))
                hipLaunchKernelGGL((blend_fwd_wave_kernel<C, decltype(xm)::value, STRIDED, PARTIAL>), dim3(fwd_wave_grid(c)), dim3(64), 0,
                                   c.stream, c.img.ranges, c.bin.blend_list, c.geom.index_rec, c.vp.W, c.vp.H, c.vp.grid_x, a.features + b.c0,
                                   c.img.final_T, c.img.n_contrib, c.img.tile_consumed, c.img.tile_nsurv, a.bg + b.c0,
                                   a.out_color + b.c0 * c.HW(), a.channels, zf, c.img.run_bounds, b.real);
        });
    });
}
template <int EXTRA>
void launch_blend_fwd_wave_rgb(const Call& c, const FwdArgs& a, FwdZeroFill& zfill)
{
    const FwdZeroFill zf = std::exchange(zfill, FwdZeroFill{nullptr, 0u, nullptr, 0u});
    with_exp_mode(c.exp_mode(), [&](auto xm) {
        hipLaunchKernelGGL((blend_fwd_wave_rgb_kernel<EXTRA, decltype(xm)::value>), dim3(fwd_wave_grid(c)), dim3(64), 0, c.stream, c.img.ranges,
                           c.bin.blend_list, c.geom.index_rec, c.vp.W, c.vp.H, c.vp.grid_x, a.features, a.mask, c.geom.depths, c.img.final_T,
                           c.img.n_contrib, c.img.tile_consumed, c.img.tile_nsurv, a.bg, a.out_color, a.out_mask, a.out_depth, zf,
                           c.img.run_bounds);
    });
}

// One wave per (tile, quadrant), a work queue per XCD behind the static share (blend_bwd_wave.h).  CR: channels of the block that exist at
// compile time -- 3 of 16 for RGB, C for a whole block, 0 for the partial block of a feature (then `real` of its 16 channels exist).
// (the row stride is a compile-time constant unless the launch handles one channel block of a wider feature)
template <int C, int CR, bool MASKGRAD>
void launch_blend_bwd_wave(const Call& c, const BwdArgs& a, int c0, int real, uint32_t* queue_ctr)
{
    const uint32_t nt = c.ntiles();
    with_bools(CR == 0 || a.channels != CR, c.xexp(), [&](auto strided, auto xexp) {
        if constexpr (CR != 0 || decltype(strided)::value)
            hipLaunchKernelGGL((blend_bwd_wave_kernel<C, CR, MASKGRAD, decltype(xexp)::value, decltype(strided)::value>),
                               dim3(32u * xcd_static_len_max(nt) + 4u * xcd_queued_tiles_max(nt)), dim3(64), 0, c.stream, c.img.ranges,
                               c.bin.blend_list, c.geom.index_rec, c.img.tile_nsurv, c.vp.W, c.vp.H, c.vp.grid_x, nt, a.bg + c0, a.colors + c0,
                               c.img.final_T, c.img.n_contrib, a.dL_dpix + c0 * c.HW(), a.dL_dout_mask, c.geom.bwd_pack, a.dL_dcolor + c0,
                               queue_ctr, a.channels, real, c.img.run_bounds);
    });
}

// Features-only backward, one wave per half tile (blend_bwd_feat.h): alpha, T, dF = W^T dL and the feature-row atomics of one
// whole channel block
template <int C>
void launch_blend_bwd_feat(const Call& c, const BwdArgs& a, int c0, uint32_t* queue_ctr)
{
    const uint32_t nt = c.ntiles();
    with_bools(a.channels != C, c.xexp(), [&](auto strided, auto xexp) {
        hipLaunchKernelGGL((blend_bwd_feat_kernel<C, decltype(xexp)::value, decltype(strided)::value>),
                           dim3(16u * xcd_static_len_max(nt) + 2u * xcd_queued_tiles_max(nt)), dim3(64), 0, c.stream, c.img.ranges,
                           c.bin.blend_list, c.geom.index_rec, c.img.tile_nsurv, c.vp.W, c.vp.H, c.vp.grid_x, nt, c.img.final_T,
                           c.img.n_contrib, a.dL_dpix + c0 * c.HW(), a.dL_dcolor + c0, queue_ctr, a.channels, c.img.run_bounds);
    });
}

// The mask-only tile backward (blend_bwd.h)
void launch_mask_bwd(const Call& c, const float* dL_dout_mask)
{
    with_bool(c.xexp(), [&](auto xexp) {
        hipLaunchKernelGGL(mask_bwd_kernel<decltype(xexp)::value>, dim3(c.vp.grid_x, c.vp.grid_y), dim3(256), 0, c.stream, c.img.ranges, c.bin.blend_list,
                           c.geom.index_rec, c.img.tile_nsurv, c.vp.W, c.vp.H, c.img.final_T, c.img.n_contrib, dL_dout_mask, c.geom.bwd_pack);
    });
}

// The lift kernel (lift.h) over all K score channels at once: the range scan's XCD runs dealt statically, 4 / LIFT_NQ items per tile
template <int NB>
void launch_lift(const Call& c, int K, const float* scores, float* votes)
{
    const uint32_t run = c.longest_run ? c.longest_run : xcd_max_run(c.ntiles());
    with_bool(c.xexp(), [&](auto xexp) {
        hipLaunchKernelGGL((lift_kernel<NB, decltype(xexp)::value>), dim3(8u * (4 / LIFT_NQ) * run), dim3(64), 0, c.stream, c.img.ranges,
                           c.bin.blend_list, c.geom.index_rec, c.vp.W, c.vp.H, c.vp.grid_x, c.ntiles(), scores, votes, K, c.img.run_bounds);
    });
}
int lift_stage(const Call& c, int K, const float* scores, float* votes)
{
    {
        StageTimer t(c.stream, MI_STAGE_BLEND_FWD);
        if (K <= 16) launch_lift<1>(c, K, scores, votes);
        else if (K <= 32) launch_lift<2>(c, K, scores, votes);
        else launch_lift<4>(c, K, scores, votes);
    }
    STAGE_CHECK(c, "lift");
    return MI_RAST_OK;
}
// what mi_rast_lift and mi_rast_lift_reuse refuse alike
int check_lift_args(int P, int K, int width, int height, const float* scores, const float* votes)
{
    if (P <= 0 || width <= 0 || height <= 0) return fail(MI_RAST_ERR_INVALID, "P, width and height must be positive");
    if (K < 1 || K > MI_RAST_LIFT_MAX_CHANNELS) return fail(MI_RAST_ERR_INVALID, "lift: need 1 <= K <= 64 score channels");
    if (!scores || !votes) return fail(MI_RAST_ERR_INVALID, "lift: null scores or votes");
    return MI_RAST_OK;
}

}  // namespace

#ifdef MI_RAST_PROFILING
// ---- profiling build only (libmi_rast_prof.so, seganygaussians_amd/build.py): the comparison forwards of earlier rounds, selected by
// MI_RAST_TILE_FWD (tile-batched bf16x3 / RGB) and MI_RAST_F32_BLEND (f32 FMA chain), and the blend kernels' XCD stamps ----
// round 2's tile-batched bf16x3 forward (blend_fwd_x3.h) over one 64- or 32-channel block
template <int C>
static void launch_blend_fwd_x3(const Call& c, const FwdArgs& a, ChannelBlock b)
{
    with_bools(a.channels != C, c.xexp(), [&](auto strided, auto xexp) {
        hipLaunchKernelGGL((blend_fwd_x3_kernel<C, decltype(xexp)::value, decltype(strided)::value>), dim3(c.vp.grid_x, c.vp.grid_y), dim3(256), 0,
                           c.stream, c.img.ranges, c.bin.blend_list, c.geom.index_rec, c.vp.W, c.vp.H, a.features + b.c0, c.img.final_T,
                           c.img.n_contrib, c.img.tile_consumed, c.img.tile_nsurv, a.bg + b.c0, a.out_color + b.c0 * c.HW(), a.channels);
    });
}
// Returns whether a comparison kernel blended the image (false: the flags ask for none that exists for this input, RGB with
// MI_RAST_F32_BLEND among them: the product kernels blend).
static bool blend_fwd_comparison(const Call& c, const FwdArgs& a)
{
    const bool tile_fwd = (c.flags & MI_RAST_TILE_FWD) != 0, f32_blend = (c.flags & MI_RAST_F32_BLEND) != 0;
    if (a.mask || a.channels == 3) {
        if (!tile_fwd) return false;
        if (a.mask) launch_blend_fwd<3, 2>(c, a, ChannelBlock{0, 3, 3});
        else launch_blend_fwd<3, 0>(c, a, ChannelBlock{0, 3, 3});
        return true;
    }
    if (!tile_fwd && !f32_blend) return false;
    // (the comparison kernels have no partial 32-channel form: what is left behind the last whole block takes the tile-batched
    // 16-channel kernel, in one or two blocks)
    for_channel_blocks(a.channels, 16, [&](ChannelBlock b) {
        if (b.width == 16) launch_blend_fwd<16, 0>(c, a, b);
        else if (b.width == 32) f32_blend ? launch_blend_fwd<32, 0>(c, a, b) : launch_blend_fwd_x3<32>(c, a, b);
        else f32_blend ? launch_blend_fwd<64, 0>(c, a, b) : launch_blend_fwd_x3<64>(c, a, b);
    });
    return true;
}

// Profiling build only (tools/xcd_stamps.py; not part of include/mi_rast.h): from the blend kernels' per-wave stamps since the last reset,
// per XCD x: out[x] = latest end of a wave, out[8 + x] = earliest start, out[16 + x] = waves -- ticks of the constant 100-MHz clock.
extern "C" int mi_rast_xcd_stamps(unsigned long long* out, int reset)
{
    static std::vector<unsigned long long> h(2 * (size_t)MI_XCD_LOG_WAVES);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_xcd_log), h.size() * sizeof(unsigned long long)));
    for (int k = 0; k < 24; k++) out[k] = 0ull;
    for (size_t b = 0; b < MI_XCD_LOG_WAVES; b++) {
        const unsigned long long s0 = h[2 * b], e0 = h[2 * b + 1];
        if (s0 == 0ull || e0 == 0ull) continue;
        const int x = (int)(s0 & 7ull);
        const unsigned long long st = s0 >> 3;
        out[x] = std::max(out[x], e0);
        out[8 + x] = out[8 + x] == 0ull ? st : std::min(out[8 + x], st);
        out[16 + x]++;
    }
    if (reset) {
        std::fill(h.begin(), h.end(), 0ull);
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_xcd_log), h.data(), h.size() * sizeof(unsigned long long)));
    }
    return MI_RAST_OK;
}
#endif

extern "C" {

const char* mi_rast_last_error(void) { return g_last_error.c_str(); }
#ifndef MI_RAST_SRC_HASH
#define MI_RAST_SRC_HASH "unstamped"
#endif
// "... src:<hash>": seganygaussians_amd/build.py source_hash() of the sources, headers and flags this library was built from
const char* mi_rast_version(void) { return "mi_rast 0.3 (gfx950) src:" MI_RAST_SRC_HASH; }

int mi_rast_supported_channels(int* out, int n)
{
    int k = 0;
    for (int c = 1; c <= MAX_CHANNELS; c++, k++)
        if (k < n) out[k] = c;
    return k;
}

// CF/cuda_rasterizer/rasterizer_impl.cu:35-50
uint32_t mi_rast_get_higher_msb(uint32_t n)
{
    uint32_t msb = sizeof(n) * 4;
    uint32_t step = msb;
    while (step > 1) {
        step /= 2;
        if (n >> msb) msb += step;
        else msb -= step;
    }
    if (n >> msb) msb++;
    return msb;
}

size_t mi_rast_geometry_layout(int P, size_t* off)
{
    const size_t p = P > 0 ? (size_t)P : 1;
    Carver c;
    off[MI_GEOM_DEPTHS] = c.take(p * sizeof(float));
    off[MI_GEOM_MEANS2D] = c.take(p * sizeof(float2));
    off[MI_GEOM_CONIC_OPACITY] = c.take(p * sizeof(float4));
    off[MI_GEOM_COV3D] = c.take(p * 6 * sizeof(float));
    off[MI_GEOM_RGB] = c.take(p * 3 * sizeof(float));
    off[MI_GEOM_CLAMPED] = c.take(p * 3);
    off[MI_GEOM_TILES_TOUCHED] = c.take(p * sizeof(uint32_t));
    off[MI_GEOM_DEPTH_KEY] = c.take(p * sizeof(uint32_t));
    off[MI_GEOM_INDEX_REC] = c.take(p * sizeof(BlendRec));
    off[MI_GEOM_CULL_COUNTER] = c.take(16);
    off[MI_GEOM_BAND_BITS] = c.take((size_t)MAX_BANDS * ((p + 63) / 64) * sizeof(unsigned long long));
    off[MI_GEOM_BWD_PACK] = c.take(bwd_pack_bytes((int)p));  // + the backward's work-queue counters, one set per channel block
    return c.off;
}
size_t mi_rast_image_layout(int width, int height, size_t* off)
{
    const size_t n = (size_t)width * height > 0 ? (size_t)width * height : 1;
    const size_t tiles = (size_t)((width + TILE_X - 1) / TILE_X) * ((height + TILE_Y - 1) / TILE_Y);
    Carver c;
    off[MI_IMG_FINAL_T] = c.take(n * sizeof(float));
    off[MI_IMG_N_CONTRIB] = c.take(n * sizeof(uint32_t));
    off[MI_IMG_RANGES] = c.take((tiles ? tiles : 1) * sizeof(uint2));
    off[MI_IMG_TILE_CONSUMED] = c.take((tiles ? tiles : 1) * sizeof(uint32_t));
    // tile_count holds partial[slice][tile] of the count / emit passes (bin_full.h, bin_lean.h); tile_cursor the tile totals
    constexpr int max_slices = BIN_MAX_WG;   // (the lean passes' [workgroup][tile of its band] table is far smaller: BIN_LEAN_WG x a band's tiles)
    off[MI_IMG_TILE_COUNT] = c.take((size_t)max_slices * (tiles ? tiles : 1) * sizeof(uint32_t));
    off[MI_IMG_TILE_CURSOR] = c.take((tiles ? tiles : 1) * sizeof(uint32_t));
    off[MI_IMG_NUM_RENDERED] = c.take((R_SLOTS * R_SLOT_STRIDE + 16) * sizeof(int));  // R partial sums, then {R, longest list}, then the nine run boundaries
    off[MI_IMG_TILE_NSURV] = c.take((tiles ? tiles : 1) * sizeof(uint32_t));
    return c.off;
}
size_t mi_rast_binning_layout(int R, size_t* off)
{
    const size_t r = R > 0 ? (size_t)R : 1;
    Carver c;
    // the blend list first: it is all the blend kernels (and a caller that keeps a view's lists, mi_rast_forward_reuse) need of this
    // buffer, at an offset that does not depend on R
    off[MI_BIN_BLEND_LIST] = c.take(r * sizeof(uint32_t));
    off[MI_BIN_ENTRIES] = c.take(r * sizeof(uint2));
    off[MI_BIN_SCRATCH] = c.take(r * sizeof(uint2));
    return c.off;
}

int mi_rast_profile_enable(int on)
{
    if (on && !profile_events(current_device())) return fail(MI_RAST_ERR_HIP, "hipEventCreate failed");
    g_profile.store(on != 0);
    for (int d = 0; d < MAX_DEVICES; d++)
        for (int i = 0; i < MI_STAGE_COUNT; i++) g_prof[d].used[i] = false;
    return MI_RAST_OK;
}

int mi_rast_profile_read(float* ms)
{
    const int dev = current_device();
    ProfileEvents* pe = dev >= 0 && g_prof[dev].created.load(std::memory_order_acquire) ? &g_prof[dev] : nullptr;
    for (int i = 0; i < MI_STAGE_COUNT; i++) {
        ms[i] = 0.f;
        if (pe && pe->used[i]) {
            HIP_TRY(hipEventSynchronize(pe->ev[i][1]));
            HIP_TRY(hipEventElapsedTime(&ms[i], pe->ev[i][0], pe->ev[i][1]));
            pe->used[i] = false;
        }
    }
    return MI_RAST_OK;
}

// The blend stage of a forward: CF/cuda_rasterizer/rasterizer_impl.cu:319-335 (+ the zero fills for this view's backward).  Shared by
// mi_rast_forward and mi_rast_forward_reuse.  args.features: the caller's colors_precomp, or NULL for the preprocess pass's RGB.
static int blend_forward_stage(const Call& c, const FwdArgs& args, void* features_ready_event, float* dL_dcolor_next)
{
    FwdArgs a = args;
    if (a.features == nullptr) a.features = c.geom.rgb;  // rasterizer_impl.cu:321
    if (a.mask == nullptr) a.out_mask = a.out_depth = nullptr;
    if (features_ready_event != nullptr) {
        // everything above depends on the geometry only; colors_precomp may still be in the making (mi_rast.h)
        HIP_TRY(hipStreamWaitEvent(c.stream, (hipEvent_t)features_ready_event, 0));
    }
    {
        StageTimer t(c.stream, MI_STAGE_BLEND_FWD);
        // zero-fill for the backward of this view (mi_rast.h: dL_dcolor_next, MI_RAST_PREZERO_BWD): stored by the first wave-per-quadrant
        // blend launch beside its own work (blend_fwd_wave.h); tails that are not whole 16-byte units, and everything when another
        // kernel blends, by fill commands
        FwdZeroFill zfill{nullptr, 0u, nullptr, 0u};
        {
            // The kernel takes the fill while it at most doubles the kernel's own stores (the image: 265 MB against 160 MB of
            // zeros on cfg3); beyond that the zeros are HBM time wherever they are stored, and the fill engine stores them faster
            // (cfg5, 5 M x 64 channels: 1.44 GB of zeros against a 435-MB image: blend 0.38 -> 0.67 ms with the fill on board,
            // 0.22 ms as fill commands).
            const size_t ride_limit = (size_t)a.channels * c.vp.W * c.vp.H * sizeof(float);
            size_t riding = 0;
            auto region = [&](float* ptr, size_t bytes, float4*& p, uint32_t& n16) -> int {
                if (ptr == nullptr || bytes == 0) return MI_RAST_OK;
                if ((reinterpret_cast<uintptr_t>(ptr) & 15u) != 0 || (bytes >> 4) > 0xFFFFFFFFull || riding + bytes > ride_limit) {
                    HIP_TRY(hipMemsetAsync(ptr, 0, bytes, c.stream));
                    return MI_RAST_OK;
                }
                p = reinterpret_cast<float4*>(ptr);
                n16 = (uint32_t)(bytes >> 4);
                riding += bytes;
                if (bytes & 15u) HIP_TRY(hipMemsetAsync(reinterpret_cast<char*>(ptr) + (bytes & ~(size_t)15), 0, bytes & 15u, c.stream));
                return MI_RAST_OK;
            };
            if (int rc = region(dL_dcolor_next, (size_t)c.P * a.channels * sizeof(float), zfill.a, zfill.na)) return rc;
            if (c.flags & MI_RAST_PREZERO_BWD)
                if (int rc = region(c.geom.bwd_pack, bwd_pack_bytes(c.P), zfill.b, zfill.nb)) return rc;
        }
        // Product kernels: the wave-per-quadrant forward (RGB, RGB + mask + depth, 64- and 32-channel blocks; the remainder of a feature is a
        // partial 32-channel block of the same kernel).  The comparison kernels of earlier rounds exist in the profiling build only.
#ifdef MI_RAST_PROFILING
        const bool compared = blend_fwd_comparison(c, a);
#else
        const bool compared = false;
        if (c.flags & (MI_RAST_TILE_FWD | MI_RAST_F32_BLEND))
            return fail(MI_RAST_ERR_INVALID, "MI_RAST_TILE_FWD / MI_RAST_F32_BLEND select comparison kernels of the profiling build "
                                             "(libmi_rast_prof.so: python -m seganygaussians_amd.build --profiling, MI_RAST_LIB=<path>)");
#endif
        if (compared) {}   // a comparison kernel has blended
        else if (a.mask) launch_blend_fwd_wave_rgb<2>(c, a, zfill);
        else if (a.channels == 3) launch_blend_fwd_wave_rgb<0>(c, a, zfill);
        else   // one launch per channel block
            for_channel_blocks(a.channels, 32, [&](ChannelBlock b) {
                if (b.width == 64) launch_blend_fwd_wave<64>(c, a, b, zfill);
                else launch_blend_fwd_wave<32>(c, a, b, zfill);
            });
        // no wave-per-quadrant launch took the fill (tile-batched / f32 / 16-channel kernels): fill commands
        if (zfill.na) HIP_TRY(hipMemsetAsync(zfill.a, 0, (size_t)zfill.na << 4, c.stream));
        if (zfill.nb) HIP_TRY(hipMemsetAsync(zfill.b, 0, (size_t)zfill.nb << 4, c.stream));
    }
    STAGE_CHECK(c, "render");
    return MI_RAST_OK;
}

int mi_rast_forward(mi_rast_resize_fn geometry_buffer, void* geometry_user, mi_rast_resize_fn binning_buffer,
                    void* binning_user, mi_rast_resize_fn image_buffer, void* image_user, int P, int D, int M,
                    int channels, const float* background, int width, int height, const float* means3D,
                    const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                    float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                    const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                    const float* mask, float* out_color, float* out_mask, float* out_depth, int* radii, int debug,
                    int flags, void* features_ready_event, float* dL_dcolor_next, void* stream_, int* num_rendered)
{
    if (num_rendered) *num_rendered = 0;
    if (int rc = check_forward_args(P, channels, width, height, colors_precomp, mask)) return rc;
    if (!num_rendered || !radii || !out_color) return fail(MI_RAST_ERR_INVALID, "null output pointer");

    Call c{make_view(viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, scale_modifier, width, height), (hipStream_t)stream_, debug, flags, P,
           {}, {}, {}, 0u};
    const FrontArgs front{geometry_buffer, binning_buffer, image_buffer, geometry_user, binning_user, image_user, D, M, colors_precomp != nullptr,
                          prefiltered, means3D, shs, opacities, scales, rotations, cov3D_precomp, radii};
    if (int rc = geometry_and_binning(c, front, num_rendered)) return rc;
    return blend_forward_stage(c, FwdArgs{channels, colors_precomp, mask, background, out_color, out_mask, out_depth}, features_ready_event,
                               dL_dcolor_next);
}

// Extension (no counterpart in the reference; include/mi_rast.h): the blend stage alone over the state a previous mi_rast_forward
// of the SAME geometry, camera and list mode left in its buffers.
int mi_rast_forward_reuse(int P, int channels, int R, const float* background, int width, int height, const float* colors_precomp,
                          char* geom_buffer, char* binning_buffer, const void* cached_ranges, const int* cached_words, char* img_buffer,
                          int longest_run, const float* mask, float* out_color, float* out_mask, float* out_depth, int flags,
                          void* features_ready_event, float* dL_dcolor_next, void* stream_)
{
    if (int rc = check_forward_args(P, channels, width, height, colors_precomp, mask)) return rc;
    if (!geom_buffer || !binning_buffer || !cached_ranges || !cached_words || !img_buffer || !out_color) return fail(MI_RAST_ERR_INVALID, "null pointer");
    Call c{make_blend_view(width, height), (hipStream_t)stream_, 0, flags, P, geom_from(geom_buffer, P), img_from(img_buffer, width, height),
           bin_from(binning_buffer, R), 0u};
    const uint32_t ntiles = c.ntiles();
    c.longest_run = longest_run > 0 ? std::min((uint32_t)longest_run, xcd_max_run(ntiles)) : 0u;
    {
        // the per-view words of the image buffer that the binning stages of the cached forward wrote: tile ranges, {R, longest list,
        // key bits}, the XCD run boundaries -- copied; the per-tile walk counters of the blend kernels -- zeroed (fingerprint.h)
        StageTimer t(c.stream, MI_STAGE_TILE_SCAN);
        hipLaunchKernelGGL(reuse_image_state_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, c.stream, ntiles, (const uint2*)cached_ranges,
                           cached_words, c.img.ranges, c.img.words(), c.img.tile_consumed, c.img.tile_nsurv);
    }
    STAGE_CHECK(c, "reuse image state");
    return blend_forward_stage(c, FwdArgs{channels, colors_precomp, mask, background, out_color, out_mask, out_depth}, features_ready_event,
                               dL_dcolor_next);
}

// Content fingerprints of up to MI_FP_MAX device arrays (a 64-bit sum of position-dependent word hashes each): what a caller keys
// reuse decisions on when tensors are recomputed per call (activation outputs) and identity says nothing.  Synchronous: one kernel,
// then the calling thread waits for `stream`.
int mi_rast_fingerprint(int n, const void* const* ptrs, const size_t* nbytes, uint64_t* out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n > MI_FP_MAX) return fail(MI_RAST_ERR_INVALID, "mi_rast_fingerprint: at most 8 arrays");
    if (n == 0) return MI_RAST_OK;
    const int dev = current_device();
    if (dev < 0) return fail(MI_RAST_ERR_HIP, "hipGetDevice failed (or device ordinal >= 64)");
    HostSync& hs = g_host_sync_tl[dev];
    if (!hs.init()) return fail(MI_RAST_ERR_HIP, "cannot allocate pinned host buffer / event");
    FingerprintArgs a;
    for (int k = 0; k < MI_FP_MAX; k++) {
        a.ptr[k] = k < n ? (const uint32_t*)ptrs[k] : nullptr;
        a.words[k] = k < n ? (unsigned long long)(nbytes[k] / 4) : 0ull;
        if (k < n && ((nbytes[k] & 3) || (reinterpret_cast<uintptr_t>(ptrs[k]) & 3))) return fail(MI_RAST_ERR_INVALID, "mi_rast_fingerprint: arrays of 4-byte words");
    }
    hipLaunchKernelGGL(fingerprint_kernel, dim3(FP_BLOCKS, n), dim3(256), 0, stream, a, (unsigned long long*)hs.fp_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < n; k++) {
        uint64_t sum = 0;
        for (int b = 0; b < FP_BLOCKS; b++) sum += hs.fp[k * FP_BLOCKS + b];
        out[k] = sum;
    }
    return MI_RAST_OK;
}

// The longest XCD run of tiles of the calling thread's last mi_rast_forward on the current device (what sizes the forward blend's
// grid): a caller that keeps the buffers of that forward for mi_rast_forward_reuse passes it back; 0 if unknown.
int mi_rast_last_longest_run(void)
{
    const int dev = current_device();
    return dev < 0 ? 0 : g_last_longest_run[dev];
}

int mi_rast_features_only_supported(int channels) { return channels >= 16 && channels <= 256 && channels % 16 == 0 ? 1 : 0; }

int mi_rast_backward(int P, int D, int M, int channels, int R, const float* background, int width, int height,
                     const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                     float scale_modifier, const float* rotations, const float* cov3D_precomp,
                     const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                     float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* img_buffer,
                     const float* dL_dpix, const float* dL_dout_mask, float* dL_dmean2D, float* dL_dconic,
                     float* dL_dopacity, float* dL_dcolor, float* dL_dmask, float* dL_dmean3D, float* dL_dcov3D,
                     float* dL_dsh, float* dL_dscale, float* dL_drot, int debug, int flags, void* stream_)
{
    if (P <= 0) return MI_RAST_OK;
    if (!channels_supported(channels)) return fail(MI_RAST_ERR_INVALID, "unsupported channel count (supported: 1 .. 256)");
    const bool maskgrad = dL_dmask != nullptr;
    if (maskgrad && (channels != 3 || !dL_dout_mask)) return fail(MI_RAST_ERR_INVALID, "mask gradient needs 3 channels and dL_dout_mask");
    // EXTENSION (mi_rast.h): dL_dcolor alone -- blend_bwd_feat.h instead of the full blend kernel, no geometry backward
    const bool feat_only = (flags & MI_RAST_BWD_FEATURES_ONLY) != 0;
    if (feat_only && (!mi_rast_features_only_supported(channels) || colors_precomp == nullptr || maskgrad || dL_dcolor == nullptr))
        return fail(MI_RAST_ERR_INVALID, "MI_RAST_BWD_FEATURES_ONLY needs colors_precomp, dL_dcolor and a channel count that is a multiple of 16");

    const Call c{make_view(viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, scale_modifier, width, height), (hipStream_t)stream_, debug, flags, P,
                 geom_from(geom_buffer, P), img_from(img_buffer, width, height), bin_from(binning_buffer, R), 0u};
    const GeomPtrs& geom = c.geom;
    const BwdArgs a{channels, background, colors_precomp != nullptr ? colors_precomp : geom.rgb /* rasterizer_impl.cu:389 */, dL_dpix,
                    dL_dout_mask, dL_dcolor};
    {
        StageTimer t(c.stream, MI_STAGE_BLEND_BWD);
        // behind the packed field gradients: the work-queue counters, one set of eight per channel block
        const size_t fields_bytes = (size_t)P * 8 * sizeof(float);
        uint32_t* queue_ctr = reinterpret_cast<uint32_t*>(geom.bwd_pack + (size_t)P * 8);
        // (MI_RAST_PREZERO_BWD: the forward of this view left the block zeroed, and no backward has run on it since)
        // (features only: the packed fields are not used, the counters behind them are)
        if (!(flags & MI_RAST_PREZERO_BWD)) {
            if (feat_only) HIP_TRY(hipMemsetAsync(queue_ctr, 0, bwd_pack_bytes(P) - fields_bytes, c.stream));
            else HIP_TRY(hipMemsetAsync(geom.bwd_pack, 0, bwd_pack_bytes(P), c.stream));
        }
        if (feat_only)
            for_channel_blocks(channels, 16, [&](ChannelBlock b) {
                if (b.width == 64) launch_blend_bwd_feat<64>(c, a, b.c0, queue_ctr);
                else if (b.width == 32) launch_blend_bwd_feat<32>(c, a, b.c0, queue_ctr);
                else launch_blend_bwd_feat<16>(c, a, b.c0, queue_ctr);
                queue_ctr += 8 * XCD_QUEUE_STRIDE;
            });
        else if (maskgrad) launch_blend_bwd_wave<16, 3, true>(c, a, 0, 0, queue_ctr);   // RGB, 3 of a 16-channel block, + the DEPTH variant's dL_dmask
        else if (channels == 3) launch_blend_bwd_wave<16, 3, false>(c, a, 0, 0, queue_ctr);
        else
            // one launch per channel block: the feature gradient of the block, and the block's share of the geometry gradients
            // (dL/dalpha is a sum over channels), which the launches accumulate in the packed record
            for_channel_blocks(channels, 16, [&](ChannelBlock b) {
                if (b.width == 64) launch_blend_bwd_wave<64, 64, false>(c, a, b.c0, b.real, queue_ctr);
                else if (b.width == 32) launch_blend_bwd_wave<32, 32, false>(c, a, b.c0, b.real, queue_ctr);
                else if (b.real == 16) launch_blend_bwd_wave<16, 16, false>(c, a, b.c0, b.real, queue_ctr);
                else launch_blend_bwd_wave<16, 0, false>(c, a, b.c0, b.real, queue_ctr);   // partial block: b.real of its 16 channels exist
                queue_ctr += 8 * XCD_QUEUE_STRIDE;
            });
    }
    STAGE_CHECK(c, "render backward");

    if (feat_only) return MI_RAST_OK;
    const float* cov3D_ptr = (cov3D_precomp != nullptr) ? cov3D_precomp : geom.cov3D;  // rasterizer_impl.cu:411
    {
        StageTimer t(c.stream, MI_STAGE_GEOM_BWD);
        // (antialiased forward: the kernel also reads the w = opacity * h that forward stored, antialias.h)
        with_bool(c.antialias(), [&](auto aa) {
            typename GeomBwdPack<decltype(aa)::value>::type pack;
            if constexpr (decltype(aa)::value) pack = GeomBwdPackAA{geom.bwd_pack, geom.conic_opacity};
            else pack = geom.bwd_pack;
            hipLaunchKernelGGL(geometry_bwd_kernel<decltype(aa)::value>, dim3((P + 255) / 256), dim3(256), 0, c.stream, P, D, M, means3D, radii, shs,
                               geom.clamped, scales, rotations, cov3D_ptr, c.vp, pack, dL_dmean2D, dL_dconic, dL_dopacity,
                               dL_dmask, dL_dmean3D, dL_dcolor, dL_dcov3D, dL_dsh, dL_dscale, dL_drot);
        });
    }
    STAGE_CHECK(c, "preprocess backward");
    return MI_RAST_OK;
}

int mi_rast_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                         uint8_t* present, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P <= 0) return MI_RAST_OK;
    const ViewParams vp = make_view(viewmatrix, projmatrix, nullptr, 1.f, 1.f, 1.f, 16, 16);
    hipLaunchKernelGGL(check_frustum_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, vp, present);
    HIP_TRY(hipGetLastError());
    return MI_RAST_OK;
}

int mi_rast_mask_forward(mi_rast_resize_fn geometry_buffer, void* geometry_user, mi_rast_resize_fn binning_buffer,
                         void* binning_user, mi_rast_resize_fn image_buffer, void* image_user, int P, int width,
                         int height, const float* means3D, const float* opacities, const float* mask,
                         const float* scales, float scale_modifier, const float* rotations,
                         const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, float tan_fovx,
                         float tan_fovy, int prefiltered, float* out_mask, int* radii, int debug, int flags,
                         void* stream_, int* num_rendered)
{
    if (num_rendered) *num_rendered = 0;
    if (P <= 0 || width <= 0 || height <= 0) return fail(MI_RAST_ERR_INVALID, "P, width and height must be positive");
    if (!num_rendered || !radii || !out_mask || !mask) return fail(MI_RAST_ERR_INVALID, "null pointer");
    Call c{make_view(viewmatrix, projmatrix, nullptr, tan_fovx, tan_fovy, scale_modifier, width, height), (hipStream_t)stream_, debug, flags, P,
           {}, {}, {}, 0u};
    // DEPTH/cuda_rasterizer/rasterizer_impl.cu:495-521: shs = nullptr, colours "given" (dummy pointer)
    const FrontArgs front{geometry_buffer, binning_buffer, image_buffer, geometry_user, binning_user, image_user, 0, 0, 1, prefiltered,
                          means3D, nullptr, opacities, scales, rotations, cov3D_precomp, radii};
    if (int rc = geometry_and_binning(c, front, num_rendered)) return rc;
    {
        StageTimer t(c.stream, MI_STAGE_BLEND_FWD);
        launch_blend_fwd<0, 1>(c, FwdArgs{0, nullptr, mask, nullptr, nullptr, out_mask, nullptr}, ChannelBlock{0, 0, 0});
    }
    STAGE_CHECK(c, "render_mask");
    return MI_RAST_OK;
}

int mi_rast_mask_backward(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                          char* img_buffer, const float* dL_dout_mask, float* dL_dmask, int debug, int flags, void* stream_)
{
    if (P <= 0) return MI_RAST_OK;
    const Call c{make_blend_view(width, height), (hipStream_t)stream_, debug, flags, P, geom_from(geom_buffer, P),
                 img_from(img_buffer, width, height), bin_from(binning_buffer, R), 0u};
    {
        StageTimer t(c.stream, MI_STAGE_BLEND_BWD);
        HIP_TRY(hipMemsetAsync(c.geom.bwd_pack, 0, (size_t)P * 8 * sizeof(float), c.stream));
        launch_mask_bwd(c, dL_dout_mask);
        hipLaunchKernelGGL(unpack_mask_kernel, dim3((P + 255) / 256), dim3(256), 0, c.stream, P, c.geom.bwd_pack, dL_dmask);
    }
    STAGE_CHECK(c, "render_mask backward");
    return MI_RAST_OK;
}

// EXTENSION (include/mi_rast.h): per-Gaussian votes of K score images, the front half of mi_rast_mask_forward + the lift kernel
int mi_rast_lift(mi_rast_resize_fn geometry_buffer, void* geometry_user, mi_rast_resize_fn binning_buffer, void* binning_user,
                 mi_rast_resize_fn image_buffer, void* image_user, int P, int K, int width, int height, const float* means3D,
                 const float* opacities, const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy, int prefiltered, const float* scores,
                 float* votes, int* radii, int debug, int flags, void* stream_, int* num_rendered)
{
    if (num_rendered) *num_rendered = 0;
    if (int rc = check_lift_args(P, K, width, height, scores, votes)) return rc;
    if (!num_rendered || !radii) return fail(MI_RAST_ERR_INVALID, "null output pointer");
    if (!geometry_buffer || !binning_buffer || !image_buffer) return fail(MI_RAST_ERR_INVALID, "lift: null buffer callback");
    Call c{make_view(viewmatrix, projmatrix, nullptr, tan_fovx, tan_fovy, scale_modifier, width, height), (hipStream_t)stream_, debug, flags, P,
           {}, {}, {}, 0u};
    const FrontArgs front{geometry_buffer, binning_buffer, image_buffer, geometry_user, binning_user, image_user, 0, 0, 1, prefiltered,
                          means3D, nullptr, opacities, scales, rotations, cov3D_precomp, radii};
    if (int rc = geometry_and_binning(c, front, num_rendered)) return rc;
    if (*num_rendered == 0) return MI_RAST_OK;   // no overlap: no Gaussian blends anywhere
    return lift_stage(c, K, scores, votes);
}

int mi_rast_lift_reuse(int P, int K, int R, int width, int height, const char* geom_buffer, const char* binning_buffer,
                       const char* img_buffer, const float* scores, float* votes, int flags, void* stream_)
{
    if (int rc = check_lift_args(P, K, width, height, scores, votes)) return rc;
    if (R < 0) return fail(MI_RAST_ERR_INVALID, "lift: R must not be negative");
    if (!geom_buffer || !binning_buffer || !img_buffer) return fail(MI_RAST_ERR_INVALID, "lift: null buffer");
    if (R == 0) return MI_RAST_OK;
    // (the field pointers are carved as the writers carve them; the lift kernel's parameters are pointers to const)
    const Call c{make_blend_view(width, height), (hipStream_t)stream_, 0, flags, P, geom_from(const_cast<char*>(geom_buffer), P),
                 img_from(const_cast<char*>(img_buffer), width, height), bin_from(const_cast<char*>(binning_buffer), R), 0u};
    return lift_stage(c, K, scores, votes);
}

}  // extern "C"
