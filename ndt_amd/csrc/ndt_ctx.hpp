// ndt_ctx.hpp -- what the host-side translation units of libndt_hip.so share: the context, the error
// convention, and the internal entry points between them.
//
//   ndt_api.hip      create / destroy / upload / trace_rays / quantize: the plain C ABI of include/ndt_hip.h
//   ndt_blob.hip     scene validation, the plugins' prepare() data, hull boxes: the scene blob (host code only)
//   ndt_frame.hip    workspace + one pass of the ray pipeline over a set of primaries (render_pass)
//   ndt_probe.hip    what the diagnostics of a profiled pass print (stream / shade / exit probes, NDT_PHASE_TIMING)
//   ndt_aa.hip       Whitted's recursive anti-aliasing on top of render_pass
//   ndt_sampled.hip  -n samples > 1, lens, area lights on top of render_pass; option "sample_cap" and the sample moments of a frame
//   ndt_render.hip   ndt_hip_render*: argument checks and the choice between the three; and where every frame staged on the device is
//                    delivered (FrameView below): the file formats' refusals and the tails.  The stage files below produce
//   ndt_multi.hip    one frame over several contexts / devices
//   ndt_fit.hip      ndt_hip_fit_spheres: the bounding-sphere fits of a frame (batched Nelder-Mead), kernel and launcher
//   ndt_kd.hip       ndt_hip_build_kdtree: the kd-tree of a frame's item boxes, level by level; kernels, launcher and C ABI
//   ndt_png.hip      ndt_hip_encode_png* / ndt_hip_render_png: a frame's PNG file made on the device; kernels, launcher and C ABI
//   ndt_apng.hip     ndt_hip_apng_* / ndt_hip_render_apng_frame: a frame sequence as one animated PNG, the difference between frames
//                    found on the device; kernels, launcher and C ABI
//   ndt_jpeg.hip     ndt_hip_encode_jpeg* / ndt_hip_render_jpeg: a frame's JPEG file made on the device; kernels, launcher and C ABI
//   ndt_exr.hip      ndt_hip_encode_exr* / ndt_hip_render_exr: a frame's OpenEXR file (linear half or float samples, the map as its Z
//                    channel) made on the device; kernels, launcher and C ABI
//   ndt_features.hip  ndt_hip_render_features*: the primary hit of every pixel (object, N-D point, normal) as planes in pixel order
//   ndt_deflate.hpp  the deflate of a 32 KiB chunk that ndt_png.hip and ndt_exr.hip share (device code)
//   ndt_depth.hip    ndt_hip_depth_rgba8_device / ndt_hip_render_*_depth: the depth map of `-z` normalised and quantised on the device
//   ndt_ssaa.hip     ndt_hip_ssaa_fold_device / ndt_hip_render_ssaa*: K x K supersampling, K ordinary renders folded on the device
//   ndt_denoise.hip  ndt_hip_denoise_device / ndt_hip_render_denoised*: the edge-avoiding a-trous filter over the double framebuffer,
//                    guided by the feature planes; kernel, launcher and C ABI.  And ndt_hip_sample_variance_device / ndt_hip_vdenoise_device /
//                    ndt_hip_render_vdenoised*: the same filter with the colour weight's width taken from the frame's sample moments
//   ndt_ao.hip       ndt_hip_ao_device / ndt_hip_render_ao* / ndt_hip_render_exr_ao: ambient occlusion from the feature planes -- the
//                    sample rays, the trace kernel as it is, the fold into a plane, the plane applied to a frame; kernels and C ABI
//   ndt_shading.hpp  the arithmetic of apply_lights and get_ray_color on values, stated once for every kernel that shades: the
//                    per-bounce and light-window kernels, the frame kernel (ndt_kernels.hip, ndt_stream.hpp), k_resolve (ndt_frame.hip)
//   ndt_buffer.hpp   DeviceBuffer: the grow-only device buffers of the context and of its sinks, their one grow and free path
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <functional>
#include <string>
#include <vector>

#include "../../include/ndt_hip.h"
#include "ndt_buffer.hpp"
#include "ndt_kernels.hpp"

namespace ndt_impl {

struct CtxWorker;       // ndt_multi.hip: the thread that drives a context inside a multi-context render

} // namespace ndt_impl
using namespace ndt_impl;

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(NDT_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

// q16, the 16-bit sample of every 16-bit file: pixel_d2c's clamp (the same two comparisons in the same order) and square root,
// scaled to 65535; the sample's two bytes come back in the order a PNG file has them (most significant first) in the low half.
// The one definition: k_quantize16 (ndt_api.hip) and k_depth_finish<true> (ndt_depth.hip) both call it.
__device__ __forceinline__ unsigned int q16_file_order(double d)
{
    double m = (1.0 < d) ? 1.0 : d;
    m = (0.0 > m) ? 0.0 : m;
    const unsigned int v = (unsigned int)(unsigned short)(sqrt(m) * 65535);
    return (v >> 8) | ((v & 255u) << 8);
}

// ndt_hip_build_kdtree (ndt_kd.hip): grow-only device buffers, reused by the next build, and the last tree in its final layout
struct KdState {
    void *d_bounds = nullptr, *d_refs = nullptr, *d_nodes = nullptr, *d_slices = nullptr, *d_slice_off[2] = { nullptr, nullptr }, *d_totals = nullptr;
    size_t bounds_bytes = 0, refs_bytes = 0, nodes_bytes = 0, slices_bytes = 0, slice_off_bytes[2] = { 0, 0 }, totals_bytes = 0;
    std::vector<ndt_flat_kdnode> nodes;         // preorder
    std::vector<int32_t> leaf_refs, inf_refs;
    std::vector<double> bb_lower, bb_upper;
    int dims = 0, depth = 0, launches = 0, grows = 0;
    bool valid = false;
};

// ndt_hip_encode_png* (ndt_png.hip): grow-only device buffers, reused by the next frame
struct PngState {
    DeviceBuffer d_rgba8, d_filtered, d_row_filter, d_slots, d_meta, d_offsets, d_file, d_info;
    void *h_info = nullptr;         // pinned: the info record of the last file
    DeviceBuffer d_rgba16;          // ndt_hip_render_png16: the frame's 16-bit samples in file byte order
};

// ndt_hip_apng_* (ndt_apng.hip): the open session and its grow-only device buffers, reused by the next frame and the next session
struct ApngState {
    DeviceBuffer d_canvas;          // the previous frame: width x rows pixels
    DeviceBuffer d_frame;           // ndt_hip_apng_add, ndt_hip_render_apng_frame: the frame that arrives
    DeviceBuffer d_crop;            // a later frame's rectangle as the compact w x h image the encoder takes
    DeviceBuffer d_rows, d_plan;    // one record per row, and the plan folded from them
    void *h_plan = nullptr;         // pinned: the plan of the last frame
    bool open = false;
    int width = 0, rows = 0, n_frames = 0, delay_num = 0, delay_den = 0, n_plays = 0;
    int next_frame = 0;             // frames added so far
    unsigned seq = 0;               // the next fcTL / fdAT sequence number
};

// ndt_hip_encode_jpeg* (ndt_jpeg.hip): grow-only device buffers, reused by the next frame
struct JpegState {
    DeviceBuffer d_rgba8, d_coef, d_slots, d_meta, d_offsets, d_file, d_info;
    void *h_info = nullptr;         // pinned: the info record of the last file
};

// ndt_hip_encode_exr* (ndt_exr.hip): grow-only device buffers, reused by the next frame
struct ExrState {
    DeviceBuffer d_in;              // ndt_hip_encode_exr: the doubles (and the map behind them) that arrive from host memory
    DeviceBuffer d_packed;          // every block's bytes as the format compresses them, each block on a chunk boundary
    DeviceBuffer d_slots, d_meta, d_offsets, d_blocks, d_file, d_info;
    DeviceBuffer d_channels;        // a file with feature channels: its channel table (ndt_exr.hip:ExrChannels)
    void *h_info = nullptr;         // pinned: the info record of the last file
};

// ndt_hip_render_features*, ndt_hip_render_exr_features (ndt_features.hip): grow-only device buffers, reused by the next frame
struct FeatureState {
    DeviceBuffer d_id, d_position, d_normal, d_ray_o, d_ray_v;     // the planes of the calls that deliver to host memory or as a file
    int launches = 0;               // kernel launches of the last feature pass
};

// ndt_hip_depth_rgba8_device, ndt_hip_render_*_depth (ndt_depth.hip): grow-only device buffers, reused by the next frame
struct DepthState {
    DeviceBuffer d_records;         // one {lo, hi, bad} record per workgroup of k_depth_range, and the folded one behind them
    DeviceBuffer d_rgba8, d_depth8;     // the two 8-bit images of ndt_hip_render_*_depth
    DeviceBuffer d_rgba16, d_grey16;    // the two 16-bit images of ndt_hip_render_png16_depth (file byte order)
    void *h_result = nullptr;       // pinned: the folded record of the last map
    int launches = 0;               // kernel launches of the last map
    double finish_ms = 0.0;         // host time of the last map: launch to the folded record in host memory
};

// ndt_hip_render_ssaa* (ndt_ssaa.hip): grow-only device buffers, reused by the next frame
struct SsaaState {
    DeviceBuffer d_pass;            // one pass of the large frame: rows x K width x 4 doubles, and its depth map behind them when wanted
    DeviceBuffer d_acc;             // the frame of the calls that deliver to host memory or as a file: rows x width x 4 doubles (+ the map)
    DeviceBuffer d_rgba8, d_depth8;     // its 8-bit image (written by the last fold) and finished map
    DeviceBuffer d_rgba16, d_grey16;    // ndt_hip_render_ssaa_png16*: the 16-bit samples of the accumulator and of the map
    hipEvent_t ev[16] = {};         // around every fold launch of a frame
    int launches = 0;               // fold launches of the last frame
    int factor = 0;                 // its K
    double fold_ms = 0.0;           // their summed device time
};

// ndt_hip_denoise_device, ndt_hip_render_denoised*, ndt_hip_vdenoise_device, ndt_hip_render_vdenoised* (ndt_denoise.hip): grow-only device buffers, reused by the next frame
struct DenoiseState {
    DeviceBuffer d_ping, d_pong;    // what the iterations between the first image and the last one write: rows x width x 4 doubles each
    DeviceBuffer d_vping, d_vpong;  // ndt_hip_vdenoise_device, ndt_hip_render_vdenoised*: the same for the variance plane, rows x width doubles each
    DeviceBuffer d_moments, d_variance;     // ndt_hip_render_vdenoised*: the frame's sums of squares with its counts behind them; its variance plane
    DeviceBuffer d_frame;           // ndt_hip_render_denoised*: the frame as rendered
    DeviceBuffer d_out, d_rgba8;    // ... denoised, for the calls that deliver to host memory or as a file, and its 8-bit image
    hipEvent_t ev[12] = {};         // around every iteration's launch
    int launches = 0;               // kernel launches of the last call of either filter: the feature pass's, k_sample_variance and the iterations'
    int iterations = 0;             // iterations of the last call
    double ms = 0.0;                // their summed device time
};

// ndt_hip_ao_device, ndt_hip_render_ao*, ndt_hip_render_exr_ao (ndt_ao.hip): grow-only device buffers, reused by the next frame
struct AoState {
    DeviceBuffer d_cos;             // the cosine of every slot of a batch: per x n_primary doubles
    DeviceBuffer d_acc;             // num and den of every pixel slot between the batches of a call: 2 x n_primary doubles
    DeviceBuffer d_plane, d_dirs;   // the plane and the directions of the calls that deliver to host memory or as a file
    DeviceBuffer d_frame, d_rgba8;  // ndt_hip_render_ao_shaded*: the frame in doubles, and its 8-bit image
    hipEvent_t ev[2] = {};          // around the pass
    bool timed = false;             // ... recorded by the last call
    int launches = 0;               // kernel launches of the last call
    double ms = 0.0;                // device time of its pass
};

struct ndt_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // the light stream (lowest priority): where the per-bounce pipeline lights bounce b beside the trace launch of bounce b + 1
    // (option "light_overlap", ndt_frame.hip:FrameInFlight::light_beside).  The main stream waits for it through events of
    // ev_pool; a frame leaves nothing running on it (FrameInFlight::render joins it on every way out)
    hipStream_t light_stream = nullptr;
    const NdtKernelTable *kt = nullptr;
    int dims = 0;
    bool have_scene = false;
    double aperture_radius = 0.0;   // camera.h:46 of the uploaded scene
    int cam_type = 0;
    bool have_eyes = false, have_local_axes = false;
    bool has_area_lights = false;   // LIGHT_DISK / LIGHT_RECT: every render is stochastic (ndt.c:116-147)
    SceneDesc sd{};
    std::vector<double> blob;
    DeviceBuffer d_blob;            // the blob on the device
    int tier = 0;
    int n_shadow_lights = 0;        // segments of the shadow queue: the non-ambient lights of the largest light window
    // The scene's lights in windows of at most 64 list entries (option "light_window": 0 auto = 64, else 1 .. 64).  The lighting
    // kernels take one window at a time: a window is the scene description with its light section narrowed to the window
    // (window_desc), and a node carries its partial colour from one window to the next.  One window:
    // the scene description as uploaded, and the kernels of a scene of up to 64 lights.
    struct LightWindow {
        int first, count;                   // list entries [first, first + count)
        int n_seg;                          // ... that are not ambient: the window's segments of the shadow queue
        unsigned long long ambient_bits;    // bit l: entry first + l is ambient
    };
    int light_window = 0;
    std::vector<int> light_types;           // NDT_LIGHT_* of every list entry (build_blob)
    std::vector<LightWindow> windows;
    // workspace
    Workspace ws{};
    std::vector<void *> ws_allocs;
    std::vector<void *> sa_allocs;                  // the frame kernel's queues and counters (ensure_stream_args)
    std::vector<DeviceBuffer> pool;                 // scratch of the multi-pass renderers (AaBuffers)
    std::vector<DeviceBuffer> pool2;                // ... of a sampled render nested in an anti-aliased one
    long long ws_dims = 0;
    long long ws_slab_words = 0;
    int ws_nseg = 0;
    // the streaming frame kernel (ndt_stream.hpp): its queues and counters live beside the workspace
    // Which pipeline renders a pass (fixed at context creation: NDT_HIP_PIPELINE=auto | levels | stream).
    //   levels  one trace launch + shade launches per bounce: three wavefronts per SIMD in the trace kernel, shade kernels
    //           with the whole chip's wavefront slots -- the better one where the rays are many (1080p: 1.46 ms against 1.77);
    //   stream  the streaming frame kernel (ndt_stream.hpp): no per-bounce latency floor -- the better one for passes of up
    //           to about a million primaries (64x36: 0.64 against 0.77 ms, 480x270: 0.61 against 0.72, 960x540: 0.68 against
    //           0.85), which is also what one GPU of eight renders of a 3840x2160 frame;
    //   auto    stream up to stream_below primaries, levels above.
    int pipeline = 0;               // 0 auto, 1 levels, 2 stream
    long long stream_below = 1000000;       // where the two cross on the benchmark scene (profiles/r03_frame_time_vs_size_*.txt: 1280x720 stream 0.918 / levels 0.965 ms, 1408x792 1.054 / 1.045; the r::8 shard of a 3840x2160 frame, 1.04 M primaries: 0.977 per bounce, 1.00 streamed)
    long long stream_below_list = 30000;    // ... for passes over a list of samples (-a): 1080p -a 20,4 of the benchmark scene 27.6 -> 24.0 ms, balls 14.0 -> 12.7
    StreamArgs sa{};
    // ndt_hip_set_option / NDT_HIP_* at context creation (include/ndt_hip.h)
    bool stream_probe = false, exit_probe = false, debug_levels = false, test_small_pool = false;
    bool hull_box = true, face_box = true;
    // per-bounce pipeline, one light window: shade_finish(b) on the light stream beside the trace launch of bounce b + 1, not on the
    // main stream in front of shade_emit(b + 1) (measured: profiles/r09_light_overlap.md)
    bool light_overlap = true;
    // ... and, where that applies, the pixels of primaries that are final early finished on the light stream instead of at the end of
    // the frame: 0 off, 1 the primaries that missed (beside trace launch 1), 2 also the hit ones without a child (behind
    // shade_finish(0): measured no better than 1, the lighting behind it on the light stream starts later).
    // FrameInFlight::early_pixels_beside; measured: profiles/r10_early_pixels.md
    int early_pixels = 1;
    bool face_tree = true;          // hcubes of more than 63 faces: a hierarchy over the face boxes (ndt_device.hpp:hull_faces)
    bool face_groups = true;        // ... and an index of the faces by the set of hull axes their boxes are thin on (hull_faces)
    // per-bounce kernels: the first trace launch makes the primaries it traces (no k_primary; k_trace's PRIM variant, planar camera).
    // -1: from 4-D on (measured, 1080p, on / off: benchmark frame 1.297 / 1.304 ms, balls 0.814 / 0.821, 6-D 1.298 / 1.326, 8-D 3.25 / 3.28;
    // 3-D 0.592 / 0.582 -- the variant spills a little more than the plain kernel, which the 2N doubles a ray it does not write and
    // read back pay for from N = 4 on), 0 never, 1 always
    int fuse_primaries = -1;
    bool stream_fused = true;       // frame kernel: makes its primaries and writes its pixels itself (no k_primary / k_finish_pixels)
    bool item_sets = true;          // scenes of up to 64 items: leaf records carry item sets (ndt_blob.hip:build_blob)
    // item sets: the min_dist-free part of every gate before the walk (ndt_device.hpp:trace_kd).  0 never, 1 always, 2 (default)
    // for passes of up to gate_prepass_below primaries -- measured (profiles/r03_gate_prepass.txt): 64x36 -6 %, 480x270 -4 %,
    // 960x540 +2 %, 1080p -1 %, the 3-D scene at 1080p +2 %: it shortens the walk of a lone slow ray, and costs the busy chip
    // about what it saves
    int gate_prepass = 2;
    long long gate_prepass_below = 400000;
    bool item_boxes = true;         // global-memory tier: orthotopes carry a box in one scene-wide frame (ndt_blob.hip:scene_item_boxes)
    int leaf_scan_group = 64;       // ... when at least this many lanes share the leaf
    bool leaf_scan = true;          // global-memory tier: lanes on the same leaf stage its items through LDS (ndt_device.hpp:cls_scan)
    int leaf_history = 4;           // global-memory tier: visited = {leaf, cut} pairs per ray (VisitMask<0>); 0: the slab only; 1 .. 3: fewer pairs (tests)
    int shade_probe = -1;           // the k-th shade launch of a frame logs its wavefronts (-1: none)
    long long sa_cap = 0, sa_sh_cap = 0;
    int sa_nseg = 0;
    DeviceBuffer d_eyes;            // the two eye images of a stochastic anaglyph render (ndt_sampled.hip)
    DeviceBuffer d_fit;             // ndt_hip_fit_spheres: jobs, points and spheres of a batch (grow-only, reused across frames)
    int fit_launches = 0;           // kernel launches of the last ndt_hip_fit_spheres call
    KdState kd;                     // ndt_hip_build_kdtree
    PngState png;                   // ndt_hip_encode_png*, ndt_hip_render_png
    ApngState apng;                 // ndt_hip_apng_*, ndt_hip_render_apng_frame
    JpegState jpeg;                 // ndt_hip_encode_jpeg*, ndt_hip_render_jpeg
    ExrState exr;                   // ndt_hip_encode_exr*, ndt_hip_render_exr, ndt_hip_render_ssaa_exr
    FeatureState features;          // ndt_hip_render_features*, ndt_hip_render_exr_features
    DepthState depth;               // ndt_hip_depth_rgba8_device, ndt_hip_render_*_depth
    SsaaState ssaa;                 // ndt_hip_render_ssaa*
    DenoiseState denoise;           // ndt_hip_denoise_device, ndt_hip_render_denoised*
    AoState ao;                     // ndt_hip_ao_device, ndt_hip_render_ao*, ndt_hip_render_exr_ao
    int ao_batch = 0;               // option "ao_batch": AO samples a trace launch; 0 auto (ndt_ao.hip:AO_AUTO_SLOTS)
    DeviceBuffer d_out;             // staging of a frame in doubles (and its map behind it) for the calls that deliver to host memory
    DeviceBuffer d_shard;           // ndt_hip_render_multi: this context's rows before they are pushed into the frame
    DeviceBuffer d_image;           // ndt_hip_render_multi (host output): the assembled frame on the first context's device
    // ndt_hip_render_rgba8_async: two quantised frames in HBM, a copy stream, and per buffer the events "quantised" / "copied"
    DeviceBuffer d_rgba8[2];
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_quantised[2] = { nullptr, nullptr }, ev_copied[2] = { nullptr, nullptr };
    bool copy_pending[2] = { false, false };
    int rgba8_turn = 0;
    // ndt_hip_render_multi without peer stores: this context's staging buffer and stream ON THE FIRST CONTEXT'S DEVICE
    DeviceBuffer d_stage;
    hipStream_t stage_stream = nullptr;
    int stage_device = 0;
    int sample_cap = 0;             // option "sample_cap": the adaptive loop of the stochastic paths stops at this many samples a pixel (0: no cap)
    DeviceBuffer d_moments;         // ndt_hip_render_moments: the sums of squares and, behind them, the counts, before they are delivered
    long long sample_seed = 0;      // option "sample_seed": selects the set of random streams of the stochastic paths (0: the default set)
    int multi_path = 0;             // option "multi_path": 0 auto, 1 never staged, 2 always staged
    int multi_path_taken = 0;       // ndt_multi_path of the last multi-context frame (ndt_hip_multi_path_taken)
    ndt_impl::CtxWorker *worker = nullptr;
    int *h_counters = nullptr;      // pinned, 128 ints: the level totals a kd-tree build reads back (ndt_kd.hip)
    LevelRange *h_levels = nullptr; // pinned, NDT_MAX_LEVELS + 1
    LevelRange *h_mail = nullptr;   // mapped + coherent: bounce ranges posted by the trace launches' prologue (TraceJob::publish_level) while the frame runs
    unsigned long long *h_mail_tag = nullptr;
    LevelRange *d_mail = nullptr;   // the device's view of the two
    unsigned long long *d_mail_tag = nullptr;
    unsigned long long frame_tag = 0;
    unsigned long long *h_done = nullptr;   // mapped + coherent: the frame's closing record (k_frame_done), [7] = its tag
    unsigned long long *d_done = nullptr;
    std::vector<hipEvent_t> ev_pool;
};

namespace ndt_impl {

// ndt_blob.hip
struct HullFaces {
    // per face of the hcube, in the hull box's frame: N x { centre coordinate, half extent } -- the face's own
    // box, same derivation and margin as the hull box; possible bit f clear = face f can never be hit
    // (possible: one word per 63 faces, bit j of word c = face 63 c + j; the top bit of every word stays clear)
    std::vector<double> rows;
    std::vector<unsigned long long> possible;
    int n_faces = 0;
};
bool hcube_hull_box(const ndt_flat_scene *fs, const ndt_flat_object &o, int n, std::vector<double> &rows, HullFaces *faces = nullptr);
void hcube_face_tree(const HullFaces &hf, int n, std::vector<double> &rows, std::vector<int> &level_off, int &top);
// clusters: n x { centre-, half-, centre+, half+ }; table: 2^n x { start, count } (ints) into members; face_set: the thin axes of every face
void hcube_face_groups(const HullFaces &hf, const std::vector<double> &hull_rows, int n, std::vector<double> &clusters, std::vector<int> &table,
                       std::vector<int> &face_set, std::vector<int> &members);
bool scene_item_boxes(const ndt_flat_scene *fs, int n, std::vector<double> &frame, std::vector<double> &rows, std::vector<char> &has);
// What check_scene learns on its way and build_blob needs: the kd nodes in preorder and the tree's depth (root = level 1).
struct SceneFacts {
    std::vector<int> kd_order;
    int kd_depth = 0;
};
// Every structural rule of include/ndt_hip.h "What upload accepts", stated once (ndt_hip_check_scene, ndt_hip_upload_scene).
int check_scene(const ndt_flat_scene *fs, SceneFacts *facts);
// Lays out a scene check_scene passed; what it decides depends on the context's options alone, and it cannot fail.
void build_blob(ndt_hip_ctx *ctx, const ndt_flat_scene *fs, const SceneFacts &facts);
// The context without a scene: have_scene false and every field an upload derives from a scene back at its initial value.
void drop_scene(ndt_hip_ctx *ctx);
// splits the uploaded scene's lights into windows of ctx->light_window entries; sets ctx->windows and ctx->n_shadow_lights
void light_windows(ndt_hip_ctx *ctx);
// the scene description `sd` with its light section narrowed to window k
SceneDesc window_desc(const ndt_hip_ctx *ctx, const SceneDesc &sd, int k);

// ndt_frame.hip
void free_workspace(ndt_hip_ctx *ctx);
// both streams of the context idle: before memory that kernels of either may still use is freed
hipError_t sync_streams(ndt_hip_ctx *ctx);
int ensure_workspace(ndt_hip_ctx *ctx, long long cap, long long sh_cap);
int render_pass(ndt_hip_ctx *ctx, RenderGeom rg, bool prof, void *d_rgba, ndt_render_stats &st, void *d_depth = nullptr);
void launch_fill_black(hipStream_t s, double *rgba, long long n_pixels);
void add_stats(ndt_render_stats &acc, const ndt_render_stats &st);

// ndt_probe.hip: each reads its log back from the device and prints to stderr
void print_stream_probe(const unsigned int *wave_log, float kernel_ms);
void print_shade_probe(const unsigned int *shade_log, int shade_probe, long long finish_waves);
void print_exit_probe(const unsigned int *exit_log, int launches);
void print_phase_timing(const unsigned long long *dbg);

// ndt_multi.hip
void worker_stop(ndt_hip_ctx *ctx);
void free_stage(ndt_hip_ctx *ctx);
void free_async(ndt_hip_ctx *ctx);

// ndt_fit.hip: bounds_list_optimal for n_lists checked point lists (first[n_lists] = number of points); synchronous
int fit_spheres_device(ndt_hip_ctx *ctx, int dims, long long n_lists, const int64_t *first, const double *points, const double *point_radius,
                       double *centers, double *radii);

// ndt_kd.hip: kd_tree_build for checked item boxes (no NaN), into ctx->kd; synchronous
int build_kdtree_device(ndt_hip_ctx *ctx, int dims, int n_items, const double *lower, const double *upper, const unsigned char *finite);
void free_kd(ndt_hip_ctx *ctx);

// ndt_png.hip
void free_png(ndt_hip_ctx *ctx);
// The file of width x rows 8-bit RGBA pixels at d_rgba8 (the context's device memory, arguments checked by the caller) made in
// ctx->png.d_file and left there: the encoder's 4 launches.  *zlib_bytes: the length of its zlib stream, which starts at byte
// PNG_ZLIB_AT of the file.  Returns when the file is complete.
constexpr int PNG_ZLIB_AT = 41;
int png_file_device(ndt_hip_ctx *ctx, const char *who, const void *d_rgba8, int32_t width, int32_t rows, long long *zlib_bytes);
// CRC-32 (the PNG polynomial)
unsigned crc32_of(const unsigned char *p, size_t len);

// ndt_apng.hip
void free_apng(ndt_hip_ctx *ctx);

// ndt_jpeg.hip
void free_jpeg(ndt_hip_ctx *ctx);

// ndt_exr.hip
void free_exr(ndt_hip_ctx *ctx);

// The file of ndt_hip_encode_exr_features_device with the FLOAT channel AO from the rows x width doubles at d_ao (device memory)
// between A and B; features may be 0 (d_planes is then not read)
int exr_encode_ao_device(ndt_hip_ctx *ctx, const char *who, const void *d_rgba, const void *d_depth, const ndt_feature_planes *d_planes,
                         const void *d_ao, int dims, int features, int32_t width, int32_t rows, const ndt_exr_params *ep, uint8_t *out,
                         int64_t cap, ndt_exr_stats *stats);

// ndt_features.hip
void free_features(ndt_hip_ctx *ctx);
// What the feature entries refuse, under the name `who`, before any device work: NULL arguments, no scene, bad geometry, and the
// frames that have no single primary ray a pixel (recursive_aa, samples > 1, anaglyph, frame packing).  *rows: the shard's
int features_check(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, int *rows);
// The feature pass of the rows `p` selects on the context's stream (arguments checked by features_check): the planes of `dst` that
// are not NULL -- device memory -- are written.  Not synchronised.
int features_pass(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, const ndt_feature_planes &dst);
// ... into the context's own buffers, the planes of `features` (NDT_FEATURE_*; with_rays: the rays too); *own names them
int features_own(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, int features, bool with_rays, ndt_feature_planes *own);

// ndt_depth.hip
void free_depth(ndt_hip_ctx *ctx);

// ndt_render.hip: delivery.  A stage (the plain render, ndt_ssaa.hip, ndt_denoise.hip, ndt_ao.hip) produces a frame into buffers of
// its own and names it; a tail takes it to the sink.  An entry is: the stage's refusal, the sink's refusal, produce, one tail.
#pragma GCC visibility push(hidden)     // (the library's dynamic symbol table stays as it was)
struct FrameView {
    const void *d_rgba;         // rows x width x 4 doubles, complete or queued on the context's stream
    const void *d_depth;        // rows x width doubles of map, or nullptr
    const void *d_rgba8;        // the 8-bit image where the producer has written it already (the last k_ssaa_fold), else nullptr
    int32_t width, rows;
    size_t pixels() const { return (size_t)rows * (size_t)width; }
};
// the plain frame (and its map) into ctx->d_out; v->rows = 0: no pixels, nothing made, the render call's word on `p` comes back
int render_plain_own(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, bool want_depth, ndt_render_stats *stats, FrameView *v);
// what ndt_hip_render_moments* refuse under the name `who`, before any device work: recursive_aa, anaglyph, frame packing
int moments_refuse(const char *who, const ndt_render_params *p);
// what a file sink refuses before the render: a shard without rows, then a size beyond the format's bound (PNG: bpp 4, 8, 2)
int refuse_empty_shard(const char *who, int rows);
int refuse_png(const char *who, int32_t width, int32_t rows, int bpp);
int refuse_jpeg(const char *who, int32_t width, int32_t rows, const ndt_jpeg_params *jp);
int refuse_exr(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_exr_params *ep, int with_depth, uint8_t *out, int *rows);
// The tails: each returns when the sink has its bytes.  The DeviceBuffers are the calling stage's own and stay so: a tail reserves
// and fills them (stage8 only where v.d_rgba8 is not set).  stage_depth8 / depth_png given: the map too, as bytes or as a file
int deliver_doubles(ndt_hip_ctx *ctx, const FrameView &v, double *rgba, double *depth);
int deliver_rgba8(ndt_hip_ctx *ctx, const char *who, FrameView v, DeviceBuffer &stage8, uint8_t *rgba8, DeviceBuffer *stage_depth8 = nullptr,
                  uint8_t *depth8 = nullptr, double *range_out = nullptr);
int deliver_png(ndt_hip_ctx *ctx, const char *who, FrameView v, DeviceBuffer &stage8, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                DeviceBuffer *stage_depth8 = nullptr, uint8_t *depth_png = nullptr, int64_t depth_cap = 0, uint8_t *depth8 = nullptr,
                double *range_out = nullptr);
int deliver_png16(ndt_hip_ctx *ctx, const char *who, const FrameView &v, DeviceBuffer &stage16, DeviceBuffer &stage_grey16, uint8_t *png,
                  int64_t cap, uint8_t *depth_png, int64_t depth_cap, ndt_png_stats *stats, double *range_out);
int deliver_jpeg(ndt_hip_ctx *ctx, const char *who, FrameView v, DeviceBuffer &stage8, const ndt_jpeg_params *jp, uint8_t *jpg,
                 int64_t cap, ndt_jpeg_stats *stats);
int deliver_exr(ndt_hip_ctx *ctx, const FrameView &v, const ndt_exr_params *ep, uint8_t *out, int64_t cap, ndt_exr_stats *stats);
#pragma GCC visibility pop

// ndt_ssaa.hip
void free_ssaa(ndt_hip_ctx *ctx);
// ndt_hip_render_ssaa_rgba8 (its refusals under the name `who`) without the download: *d_rgba8 is the frame's 8-bit image in the
// context's device memory, written by the last fold, valid until the next supersampled frame
int render_ssaa_rgba8_own(ndt_hip_ctx *ctx, const char *who, const ndt_render_params *p, int K, ndt_render_stats *stats, const void **d_rgba8);

// ndt_denoise.hip
void free_denoise(ndt_hip_ctx *ctx);

// ndt_ao.hip
void free_ao(ndt_hip_ctx *ctx);

// ndt_aa.hip / ndt_sampled.hip
int render_antialiased(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, ndt_render_stats &total, void *d_depth = nullptr);
// ndt_render.hip: true anaglyph (ndt.c:643-647) of two eye images, n_pixels x rgba each
void launch_anaglyph(hipStream_t s, const double *left, const double *right, double *out, long long n_pixels);
// mo (ndt_hip_render_moments*; not for an anaglyph): where the loop also leaves what it consumed -- device memory
struct SampleMoments {
    void *d_count;              // [n_pixels] int32: samples consumed
    void *d_sum_sq;             // [3][n_pixels] doubles: the sums of their squared r, g, b
};
int render_sampled(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, ndt_render_stats &total, void *d_depth = nullptr,
                   const SampleMoments *mo = nullptr);
// get_pixel_color's adaptive loop (ndt.c:488-568) for a LIST of image positions (2 doubles each, pixels of an img_w x img_h
// image): the samples of a stochastic anti-aliased render (a lens, area lights).  No jitter (ndt.c:505: not in this mode).
struct SampledList {
    const double *d_pos;
    long long n_pos;
    int img_w, img_h, aspect_w, aspect_h;
};
int render_sampled_list(ndt_hip_ctx *ctx, const ndt_render_params *p, const SampledList &sl, int eye, int stereo, unsigned long long salt,
                        void *d_rgba, ndt_render_stats &total);

// One slot of a device-side list for every lane that wants one, with ONE atomic per wavefront (a counter serves ~150
// returning atomics per us: a list appended to by every thread of a 2-million-thread launch queues for milliseconds).
// Every lane of the wavefront has to call it.
__device__ __forceinline__ int wave_append(int *counter, bool want)
{
    const unsigned long long vote = __ballot(want);
    if (vote == 0ull) return 0;
    const int lane = __lane_id(), leader = __ffsll((long long)vote) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(vote));
    base = __shfl(base, leader, 64);
    return base + __popcll(vote & ((1ull << lane) - 1ull));
}

// The same for a whole workgroup (up to 1024 lanes): ONE atomic on the counter a workgroup, its wavefronts' places handed out
// through LDS.  Every lane of the workgroup must call it.  (Atomics on one address complete at about a hundred million a
// second: a kernel of 32 000 wavefronts that appends once per wavefront spends 0.3 ms on its counter, whatever else it does.)
__device__ __forceinline__ int block_append(int *counter, bool want)
{
    __shared__ int wave_count[16], wave_base[16];
    const unsigned long long vote = __ballot(want);
    const int lane = __lane_id(), wave = (int)(threadIdx.x >> 6), n_waves = (int)((blockDim.x + 63) >> 6);
    if (lane == 0) wave_count[wave] = __popcll(vote);
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < n_waves; ++w) { wave_base[w] = total; total += wave_count[w]; }
        const int base = total > 0 ? atomicAdd(counter, total) : 0;
        for (int w = 0; w < n_waves; ++w) wave_base[w] += base;
    }
    __syncthreads();
    return wave_base[wave] + __popcll(vote & ((1ull << lane) - 1ull));
}

// ... and for lanes that append `n` items each (0 <= n): returns the lane's first slot; its items are adjacent
__device__ __forceinline__ int block_append_n(int *counter, int n)
{
    __shared__ int wave_count_n[16], wave_base_n[16];
    const int lane = __lane_id(), wave = (int)(threadIdx.x >> 6), n_waves = (int)((blockDim.x + 63) >> 6);
    int incl = n;                                   // inclusive prefix sum over the wavefront
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_count_n[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < n_waves; ++w) { wave_base_n[w] = total; total += wave_count_n[w]; }
        const int base = total > 0 ? atomicAdd(counter, total) : 0;
        for (int w = 0; w < n_waves; ++w) wave_base_n[w] += base;
    }
    __syncthreads();
    return wave_base_n[wave] + incl - n;
}

// Scratch buffers of the multi-pass renderers (anti-aliasing levels, sample rounds, anaglyph eyes).  The
// requests of a frame come in the same order every frame, so the k-th request reuses the k-th
// allocation of the context's pool (grown when too small) instead of a hipMalloc / hipFree pair, each of
// which synchronises the device.
struct AaBuffers {
    ndt_hip_ctx *ctx;
    std::vector<DeviceBuffer> *from;
    size_t next = 0;
    explicit AaBuffers(ndt_hip_ctx *c, bool nested = false) : ctx(c), from(nested ? &c->pool2 : &c->pool) {}
    template <typename T> int get(T **ptr, size_t count)
    {
        if (next == from->size()) from->push_back(DeviceBuffer());
        DeviceBuffer &slot = (*from)[next++];
        // with head room: frame-to-frame counts vary
        const int rc = slot.reserve((count > 0 ? count : 1) * sizeof(T), ctx->stream, "scratch of a multi-pass render", true);
        *ptr = slot.as<T>();
        return rc;
    }
};

} // namespace ndt_impl
