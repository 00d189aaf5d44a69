/* ndt_render.c -- render_image (reference ndt.c:900) for this host model: flatten, upload,
 * render on the GPU through the C ABI of include/ndt_hip.h.  No CPU rendering exists here. */
#include "ndt_host_internal.h"
#include <time.h>

/* GPU contexts (stream + workspace) of the calling host thread: frames rendered from different threads overlap on the
 * GPU, or run on different GPUs (ndt_render_use_device); one frame may be spread over several (ndt_render_use_devices) */
#define NDT_MAX_CTX 64
static __thread ndt_hip_ctx *g_ctx[NDT_MAX_CTX];
static __thread int g_n_ctx = 0;            /* contexts that exist */
static __thread int g_want_ctx = 1;         /* contexts a frame is spread over */
static __thread int g_first_device = 0;
static __thread int g_paths_said = 0;
static __thread int g_sample_cap = 0;       /* the "sample_cap" the thread's contexts were last given */

static void drop_contexts(void)
{
    for (int k = 0; k < g_n_ctx; ++k) ndt_hip_destroy(g_ctx[k]);
    g_n_ctx = 0;
    g_paths_said = 0;
    g_sample_cap = 0;
}

void ndt_render_use_device(int device)
{
    if (device < 0) device = 0;
    if (g_want_ctx != 1 || g_first_device != device) drop_contexts();
    g_want_ctx = 1;
    g_first_device = device;
}

void ndt_render_use_devices(int n_contexts)
{
    if (n_contexts < 1) n_contexts = 1;
    if (n_contexts > NDT_MAX_CTX) n_contexts = NDT_MAX_CTX;
    if (g_want_ctx != n_contexts || g_first_device != 0) drop_contexts();
    g_want_ctx = n_contexts;
    g_first_device = 0;
}

/* the thread's contexts, created on first use: context k on device (first + k) mod device count */
static int have_contexts(void)
{
    int n_dev = ndt_hip_device_count();
    if (n_dev < 1) n_dev = 1;               /* ndt_hip_create then says why there is no device */
    while (g_n_ctx < g_want_ctx) {
        if (ndt_hip_create((g_first_device + g_n_ctx) % n_dev, &g_ctx[g_n_ctx]) != NDT_OK) return 0;
        ++g_n_ctx;
    }
    return 1;
}

/* ---- the frame's bounding-sphere fits on the GPU (ndt_hip_fit_spheres) */
static int g_fit_on_gpu = 0;                /* process-wide, set before any frame: `ndt_hip --fit gpu` */
static __thread int g_fit_launches = 0;

void ndt_render_fit_on_gpu(int on) { g_fit_on_gpu = on != 0; }

static int device_fit(void *arg, int dims, int64_t n_lists, const int64_t *first, const double *points, const double *point_radius,
                      double *centers, double *radii, char *err, int err_len)
{
    ndt_hip_ctx *ctx = (ndt_hip_ctx *)arg;
    const int rc = ndt_hip_fit_spheres(ctx, dims, n_lists, first, points, point_radius, centers, radii);
    if (rc != NDT_OK) {
        snprintf(err, (size_t)err_len, "bounding spheres on the GPU: %s", ndt_hip_last_error());
        return rc;
    }
    g_fit_launches += ndt_hip_fit_launches(ctx);
    return 0;
}

/* ---- the frame's kd-tree on the GPU (ndt_hip_build_kdtree) */
static int g_kd_on_gpu = 0;                 /* process-wide, set before any frame: `ndt_hip --kd gpu` */
static __thread int g_kd_launches = 0;

void ndt_render_kd_on_gpu(int on) { g_kd_on_gpu = on != 0; }

static int device_kd(void *arg, int dims, int n_items, const double *lower, const double *upper, const unsigned char *finite,
                     ndt_host_kdtree *out, char *err, int err_len)
{
    ndt_hip_ctx *ctx = (ndt_hip_ctx *)arg;
    ndt_kd_counts c;
    int rc = ndt_hip_build_kdtree(ctx, dims, n_items, lower, upper, finite, &c);
    if (rc == NDT_OK) {
        memset(out, 0, sizeof(*out));
        out->n_kd_nodes = c.n_kd_nodes; out->n_leaf_refs = c.n_leaf_refs; out->n_inf = c.n_inf; out->depth = c.depth;
        out->nodes = (ndt_flat_kdnode *)calloc((size_t)c.n_kd_nodes, sizeof(ndt_flat_kdnode));
        out->leaf_refs = (int32_t *)malloc((size_t)(c.n_leaf_refs > 0 ? c.n_leaf_refs : 1) * sizeof(int32_t));
        out->inf_refs = (int32_t *)malloc((size_t)(c.n_inf > 0 ? c.n_inf : 1) * sizeof(int32_t));
        out->bb_lower = (double *)malloc((size_t)dims * sizeof(double));
        out->bb_upper = (double *)malloc((size_t)dims * sizeof(double));
        rc = ndt_hip_kdtree_fetch(ctx, out->nodes, out->leaf_refs, out->inf_refs, out->bb_lower, out->bb_upper);
    }
    if (rc != NDT_OK) {
        snprintf(err, (size_t)err_len, "kd-tree on the GPU: %s", ndt_hip_last_error());
        return rc;
    }
    g_kd_launches += c.launches;
    return 0;
}

int ndt_flatten_scene_gpu(scene *scn, ndt_flat_builder *fb, char *err, int err_len, int threads, int fit_on_gpu, int kd_on_gpu,
                          ndt_fit_stats *stats, ndt_kd_stats *kd_stats)
{
    ndt_fit_stats local;
    if (!stats) stats = &local;
    memset(fb, 0, sizeof(*fb));
    /* the contexts before the scene: context 0 does the work (-j K: every worker thread has its own; -g N: the first of N) */
    if ((fit_on_gpu || kd_on_gpu) && !have_contexts()) {
        snprintf(err, (size_t)err_len, "%s on the GPU: %s", fit_on_gpu ? "bounding spheres" : "kd-tree", ndt_hip_last_error());
        return -1;
    }
    g_fit_launches = 0;
    g_kd_launches = 0;
    if (ndt_flatten_scene_with(scn, fb, err, err_len, threads, fit_on_gpu ? device_fit : NULL, fit_on_gpu ? g_ctx[0] : NULL, stats,
                               kd_on_gpu ? device_kd : NULL, kd_on_gpu ? g_ctx[0] : NULL, kd_stats) != 0) return -1;
    if (fit_on_gpu)
        printf("fitted %lld bounding spheres on GPU %d in %d launches\n", (long long)stats->spheres, ndt_hip_device(g_ctx[0]), g_fit_launches);
    if (kd_on_gpu)
        printf("built kd-tree of %d nodes on GPU %d in %d launches\n", fb->n_nodes, ndt_hip_device(g_ctx[0]), g_kd_launches);
    return 0;
}

int ndt_flatten_scene_gpu_fit(scene *scn, ndt_flat_builder *fb, char *err, int err_len, int threads, ndt_fit_stats *stats)
{
    return ndt_flatten_scene_gpu(scn, fb, err, err_len, threads, 1, 0, stats, NULL);
}

int ndt_render_image(scene *scn, int width, int height, int threads, int max_optic_depth, double *rgba)
{
    return ndt_render_image_aa(scn, width, height, threads, -1, -1, max_optic_depth, rgba);
}

/* render_image with the reference's `-a diff,depth` (recursive_aa, ndt.c:44, 1039-1087); aa_depth < 0 = plain: the frame request
 * of the reference's call shape (mono, one sample, specular on), its doubles copied into the caller's image */
int ndt_render_image_aa(scene *scn, int width, int height, int threads, int aa_diff, int aa_depth, int max_optic_depth,
                        double *rgba)
{
    ndt_frame_request rq;
    ndt_frame f;
    memset(&rq, 0, sizeof(rq));         /* colour: doubles, map: none */
    rq.width = width; rq.height = height; rq.samples = 1; rq.threads = threads; rq.aa_diff = aa_diff; rq.aa_depth = aa_depth;
    rq.specular = 1; rq.max_optic_depth = max_optic_depth; rq.ssaa = 1;
    if (!ndt_render_frame(scn, &rq, &f)) return 0;
    memcpy(rgba, f.rgba, (size_t)width * height * 4 * sizeof(double));
    ndt_frame_free(&f);
    return 1;
}

/* ---- the lines a frame's device work is reported with (stdout: tests and people read them) */
static void say_png(const ndt_png_stats *ps, const char *what)
{
    printf("compressed %s of %lld bytes on GPU %d in %d launches\n", what, (long long)ps->png_bytes, ndt_hip_device(g_ctx[0]), ps->launches);
}

static void say_jpeg(const ndt_jpeg_stats *js)
{
    printf("encoded JPEG of %lld bytes on GPU %d in %d launches\n", (long long)js->jpeg_bytes, ndt_hip_device(g_ctx[0]), js->launches);
}

static void say_map(const double *range)
{
    printf("finished depth map [%.17g, %.17g] on GPU %d in %d launches\n", range[0], range[1], ndt_hip_device(g_ctx[0]),
           ndt_hip_depth_launches(g_ctx[0]));
}

static void say_ssaa(int K, int launches)
{
    printf("supersampled %dx%d on GPU %d in %d launches\n", K, K, ndt_hip_device(g_ctx[0]), launches);
}

static int out_of_memory(void)
{
    fprintf(stderr, "ndt_render_frame: out of memory\n");
    return 0;
}

/* ---- an 8-bit image in host memory as a PNG or JPEG file made on the GPU (ndt_hip_encode_png / ndt_hip_encode_jpeg) */
int ndt_encode_image_png(const unsigned char *rgba8, int width, int height, unsigned char **png, long long *png_bytes, double *encode_ms)
{
    const int64_t cap = ndt_hip_png_bound(width, height);
    ndt_png_stats ps;
    *png = NULL;
    *png_bytes = 0;
    if (cap < 0) {
        fprintf(stderr, "ndt_encode_image_png: no PNG of %d x %d: the size is empty or its filtered stream exceeds 2^31 - 1 bytes\n", width, height);
        return 0;
    }
    unsigned char *buf = (unsigned char *)malloc((size_t)cap);
    if (!buf || !have_contexts() || ndt_hip_encode_png(g_ctx[0], rgba8, width, height, buf, cap, &ps) != NDT_OK) {
        fprintf(stderr, "ndt_encode_image_png: %s\n", buf ? ndt_hip_last_error() : "out of memory");
        free(buf);
        return 0;
    }
    say_png(&ps, "PNG");
    *png = buf;
    *png_bytes = ps.png_bytes;
    if (encode_ms) *encode_ms = ps.encode_ms;
    return 1;
}

static ndt_jpeg_params jpeg_params_of(int quality, int sampling)
{
    ndt_jpeg_params jp;
    memset(&jp, 0, sizeof(jp));
    jp.quality = quality;
    jp.sampling = sampling;
    return jp;
}

int ndt_encode_image_jpeg(const unsigned char *rgba8, int width, int height, int quality, int sampling, unsigned char **jpg, long long *jpg_bytes,
                          double *encode_ms)
{
    const ndt_jpeg_params jp = jpeg_params_of(quality, sampling);
    const int64_t cap = ndt_hip_jpeg_bound(width, height, &jp);
    ndt_jpeg_stats js;
    *jpg = NULL;
    *jpg_bytes = 0;
    if (cap < 0) {
        fprintf(stderr, "ndt_encode_image_jpeg: no JPEG of %d x %d at quality %d, sampling %d\n", width, height, quality, sampling);
        return 0;
    }
    unsigned char *buf = (unsigned char *)malloc((size_t)cap);
    if (!buf || !have_contexts() || ndt_hip_encode_jpeg(g_ctx[0], rgba8, width, height, &jp, buf, cap, &js) != NDT_OK) {
        fprintf(stderr, "ndt_encode_image_jpeg: %s\n", buf ? ndt_hip_last_error() : "out of memory");
        free(buf);
        return 0;
    }
    say_jpeg(&js);
    *jpg = buf;
    *jpg_bytes = js.jpeg_bytes;
    if (encode_ms) *encode_ms = js.encode_ms;
    return 1;
}

/* ---- the run's frames as one animated PNG (ndt_hip_apng_*; `ndt_hip --apng`): opened and closed around the frames */
int ndt_apng_begin(int width, int height, int n_frames, int fps)
{
    if (fps < 1 || fps > 1000) {
        fprintf(stderr, "ndt_apng_begin: %d frames a second is outside 1 .. 1000\n", fps);
        return 0;
    }
    if (g_want_ctx > 1) {
        fprintf(stderr, "ndt_apng_begin: the frames of an animated PNG meet one canvas on one GPU context, not on %d\n", g_want_ctx);
        return 0;
    }
    if (!have_contexts() || ndt_hip_apng_begin(g_ctx[0], width, height, n_frames, 1, fps, 0) != NDT_OK) {
        fprintf(stderr, "ndt_apng_begin: %s\n", ndt_hip_last_error());
        return 0;
    }
    return 1;
}

int ndt_apng_end(unsigned char *out, long long *n_bytes)
{
    int64_t n = 0;
    *n_bytes = 0;
    if (!have_contexts() || ndt_hip_apng_end(g_ctx[0], out, 16, &n) != NDT_OK) {
        fprintf(stderr, "ndt_apng_end: %s\n", ndt_hip_last_error());
        return 0;
    }
    *n_bytes = n;
    return 1;
}

/* ---- one frame (ndt_render_frame): each routine below brings one group of sinks into the ndt_frame; what it allocates there
 * and then fails to fill, ndt_render_frame frees */
void ndt_frame_free(ndt_frame *f)
{
    free(f->rgba);
    free(f->depth);
    free(f->rgba8);
    free(f->depth8);
    free(f->file);
    free(f->depth_file);
    memset(f, 0, sizeof(*f));
}

/* the doubles (format NDT_IMAGE_F64) or the bytes (NDT_IMAGE_RGBA8) of the frame supersampled K x K (ndt_hip_render_ssaa*) in host
 * memory: from the one context, or from several, each of which renders and folds its own cyclic row shard, context after context */
static int ssaa_image(const ndt_render_params *p, int K, int format, void *out, int *launches, double *fold_ms)
{
    const size_t px = format == NDT_IMAGE_F64 ? 4 * sizeof(double) : 4;
    *launches = 0;
    *fold_ms = 0.0;
    if (g_n_ctx == 1) {
        const int rc = format == NDT_IMAGE_F64 ? ndt_hip_render_ssaa(g_ctx[0], p, K, (double *)out, NULL, NULL)
                                               : ndt_hip_render_ssaa_rgba8(g_ctx[0], p, K, (unsigned char *)out, NULL);
        *launches = ndt_hip_ssaa_launches(g_ctx[0]);
        *fold_ms = ndt_hip_ssaa_ms(g_ctx[0]);
        return rc == NDT_OK;
    }
    const size_t row_bytes = (size_t)p->width * px;
    unsigned char *part = (unsigned char *)malloc(row_bytes * (size_t)((p->height + g_n_ctx - 1) / g_n_ctx));
    int ok = part != NULL;
    for (int k = 0; ok && k < g_n_ctx; ++k) {
        ndt_render_params q = *p;
        q.row_begin = k;
        q.row_step = g_n_ctx;
        const int rows = ndt_hip_shard_rows(p->height, k, g_n_ctx);
        if (rows < 1) continue;
        ok = (format == NDT_IMAGE_F64 ? ndt_hip_render_ssaa(g_ctx[k], &q, K, (double *)part, NULL, NULL)
                                      : ndt_hip_render_ssaa_rgba8(g_ctx[k], &q, K, part, NULL)) == NDT_OK;
        for (int r = 0; ok && r < rows; ++r)
            memcpy((unsigned char *)out + (size_t)(k + r * g_n_ctx) * row_bytes, part + (size_t)r * row_bytes, row_bytes);
        *launches += ndt_hip_ssaa_launches(g_ctx[k]);
        *fold_ms += ndt_hip_ssaa_ms(g_ctx[k]);
    }
    free(part);
    return ok;
}

/* colour in doubles or 8-bit RGBA, with the map in doubles beside the doubles if asked: rows of all the thread's contexts, except
 * that the depth map comes from the one-context call (a map is not split over devices) */
static int frame_pixels(const ndt_render_params *p, const ndt_frame_request *rq, ndt_frame *f)
{
    const int format = rq->colour == NDT_COLOUR_F64 ? NDT_IMAGE_F64 : NDT_IMAGE_RGBA8, K = rq->ssaa;
    const size_t n = (size_t)p->width * (size_t)p->height;
    void *out;
    int ok, launches = 0;
    if (format == NDT_IMAGE_F64) out = f->rgba = (double *)malloc(n * 4 * sizeof(double));
    else out = f->rgba8 = (unsigned char *)malloc(n * 4);
    if (rq->map == NDT_MAP_F64) f->depth = (double *)malloc(n * sizeof(double));
    if (!out || (rq->map == NDT_MAP_F64 && !f->depth)) return out_of_memory();
    if (rq->map == NDT_MAP_F64 && K != 1) {     /* (0, 9, ... reach the library, which says what is wrong with them) */
        ok = ndt_hip_render_ssaa(g_ctx[0], p, K, f->rgba, f->depth, NULL) == NDT_OK;
        launches = ndt_hip_ssaa_launches(g_ctx[0]);
        f->ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
    } else if (rq->map == NDT_MAP_F64)
        ok = ndt_hip_render_depth(g_ctx[0], p, f->rgba, f->depth, NULL) == NDT_OK;
    else if (K != 1)
        ok = ssaa_image(p, K, format, out, &launches, &f->ssaa_ms);
    else
        ok = ndt_hip_render_multi(g_ctx, g_n_ctx, p, format, out, NULL) == NDT_OK;
    if (ok && K != 1) say_ssaa(K, launches);
    return ok;
}

/* colour as a PNG or a JPEG file made on the GPU, plain or supersampled.  One context: the file is made where the image is, and
 * the 8-bit image never leaves the device.  Several: their rows are gathered into host memory as 8-bit pixels and encoded from
 * there on the first context */
static int frame_file(const ndt_render_params *p, const ndt_frame_request *rq, ndt_frame *f)
{
    const int png = rq->colour == NDT_COLOUR_PNG, K = rq->ssaa, width = p->width, height = p->height;
    const ndt_jpeg_params jp = jpeg_params_of(rq->jpeg_quality, rq->jpeg_sampling);
    const int64_t cap = png ? ndt_hip_png_bound(width, height) : ndt_hip_jpeg_bound(width, height, &jp);
    ndt_png_stats ps;
    ndt_jpeg_stats js;
    int ok, launches = 0;
    unsigned char *buf = f->file = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
    if (!buf) {
        if (png) fprintf(stderr, "ndt_render_frame: no PNG of %d x %d\n", width, height);
        else fprintf(stderr, "ndt_render_frame: no JPEG of %d x %d at quality %d, sampling %d\n", width, height, jp.quality, jp.sampling);
        return 0;
    }
    if (g_n_ctx == 1 && K == 1) {
        ok = (png ? ndt_hip_render_png(g_ctx[0], p, buf, cap, &ps, NULL) : ndt_hip_render_jpeg(g_ctx[0], p, &jp, buf, cap, &js, NULL)) == NDT_OK;
    } else if (g_n_ctx == 1) {
        ok = (png ? ndt_hip_render_ssaa_png(g_ctx[0], p, K, buf, cap, &ps, NULL)
                  : ndt_hip_render_ssaa_jpeg(g_ctx[0], p, K, &jp, buf, cap, &js, NULL)) == NDT_OK;
        launches = ndt_hip_ssaa_launches(g_ctx[0]);
        f->ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
    } else {
        unsigned char *rgba8 = (unsigned char *)malloc((size_t)width * height * 4);
        ok = rgba8 && (K == 1 ? ndt_hip_render_multi(g_ctx, g_n_ctx, p, NDT_IMAGE_RGBA8, rgba8, NULL) == NDT_OK
                              : ssaa_image(p, K, NDT_IMAGE_RGBA8, rgba8, &launches, &f->ssaa_ms)) &&
             (png ? ndt_hip_encode_png(g_ctx[0], rgba8, width, height, buf, cap, &ps)
                  : ndt_hip_encode_jpeg(g_ctx[0], rgba8, width, height, &jp, buf, cap, &js)) == NDT_OK;
        free(rgba8);
    }
    if (!ok) return 0;
    f->file_bytes = png ? ps.png_bytes : js.jpeg_bytes;
    f->file_ms = png ? ps.encode_ms : js.encode_ms;
    if (png) say_png(&ps, "PNG");
    else say_jpeg(&js);
    if (K != 1) say_ssaa(K, launches);
    return 1;
}

/* colour as 8-bit RGBA or a PNG file beside the map of -z finished on the GPU, as 8-bit grey or a PNG file (one context, like
 * every frame with a map).  The plain frame's files are made where the images are (ndt_hip_render_png_depth); of a supersampled
 * frame the two 8-bit images come back, and the files asked for are encoded from them */
static int frame_beside_map8(const ndt_render_params *p, const ndt_frame_request *rq, ndt_frame *f)
{
    const int width = p->width, height = p->height, K = rq->ssaa;
    const int want_png = rq->colour == NDT_COLOUR_PNG, want_depth_png = rq->map == NDT_MAP_PNG;
    const size_t bytes = (size_t)width * (size_t)height * 4;
    if (K == 1 && want_png) {
        const int64_t cap = ndt_hip_png_bound(width, height);
        ndt_png_stats ps[2];
        memset(ps, 0, sizeof(ps));
        if (cap < 0) {
            fprintf(stderr, "ndt_render_frame: no PNG of %d x %d\n", width, height);
            return 0;
        }
        f->file = (unsigned char *)malloc((size_t)cap);
        if (want_depth_png) f->depth_file = (unsigned char *)malloc((size_t)cap);
        else f->depth8 = (unsigned char *)malloc(bytes);
        if (!f->file || !(want_depth_png ? f->depth_file : f->depth8)) return out_of_memory();
        if (ndt_hip_render_png_depth(g_ctx[0], p, f->file, cap, f->depth_file, cap, f->depth8, ps, f->range, NULL) != NDT_OK) return 0;
        f->file_bytes = ps[0].png_bytes;
        f->depth_file_bytes = ps[1].png_bytes;
        f->file_ms = ps[0].encode_ms + ps[1].encode_ms;
        say_png(&ps[0], "PNG");
        if (want_depth_png) say_png(&ps[1], "depth PNG");
    } else {
        f->rgba8 = (unsigned char *)malloc(bytes);
        f->depth8 = (unsigned char *)malloc(bytes);
        if (!f->rgba8 || !f->depth8) return out_of_memory();
        if ((K == 1 ? ndt_hip_render_rgba8_depth(g_ctx[0], p, f->rgba8, f->depth8, f->range, NULL)
                    : ndt_hip_render_ssaa_rgba8_depth(g_ctx[0], p, K, f->rgba8, f->depth8, f->range, NULL)) != NDT_OK) return 0;
    }
    f->depth_ms = ndt_hip_depth_ms(g_ctx[0]);
    say_map(f->range);
    if (K == 1) return 1;
    f->ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
    if (want_png) {
        if (!ndt_encode_image_png(f->rgba8, width, height, &f->file, &f->file_bytes, &f->file_ms)) return 0;
        free(f->rgba8);
        f->rgba8 = NULL;
    }
    if (want_depth_png) {
        double map_ms = 0.0;
        if (!ndt_encode_image_png(f->depth8, width, height, &f->depth_file, &f->depth_file_bytes, &map_ms)) return 0;
        f->file_ms += map_ms;
        free(f->depth8);
        f->depth8 = NULL;
    }
    say_ssaa(K, ndt_hip_ssaa_launches(g_ctx[0]));
    return 1;
}

/* colour as a PNG file of 16 bits a sample, and the map beside it as 16-bit grey if asked (ndt_hip_render_png16*,
 * ndt_hip_render_ssaa_png16*; `ndt_hip --png16`) */
static int frame_png16(const ndt_render_params *p, const ndt_frame_request *rq, ndt_frame *f)
{
    const int width = p->width, height = p->height, K = rq->ssaa, with_map = rq->map == NDT_MAP_PNG16;
    const int64_t cap = ndt_hip_png16_bound(width, height, 4), depth_cap = ndt_hip_png16_bound(width, height, 1);
    ndt_png_stats ps[2];
    int ok;
    if (g_n_ctx > 1) {
        /* (the rows of several contexts meet as 8-bit pixels or as doubles on the host: there is no 16-bit gather) */
        fprintf(stderr, "ndt_render_frame: a 16-bit PNG is made by one GPU context, not by %d\n", g_n_ctx);
        return 0;
    }
    if (cap < 0 || depth_cap < 0) {
        fprintf(stderr, "ndt_render_frame: no 16-bit PNG of %d x %d\n", width, height);
        return 0;
    }
    f->file = (unsigned char *)malloc((size_t)cap);
    if (with_map) f->depth_file = (unsigned char *)malloc((size_t)depth_cap);
    if (!f->file || (with_map && !f->depth_file)) return out_of_memory();
    if (with_map)
        ok = (K != 1 ? ndt_hip_render_ssaa_png16_depth(g_ctx[0], p, K, f->file, cap, f->depth_file, depth_cap, ps, f->range, NULL)
                     : ndt_hip_render_png16_depth(g_ctx[0], p, f->file, cap, f->depth_file, depth_cap, ps, f->range, NULL)) == NDT_OK;
    else
        ok = (K != 1 ? ndt_hip_render_ssaa_png16(g_ctx[0], p, K, f->file, cap, ps, NULL) : ndt_hip_render_png16(g_ctx[0], p, f->file, cap, ps, NULL)) == NDT_OK;
    if (!ok) return 0;
    if (K != 1) {
        f->ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
        say_ssaa(K, ndt_hip_ssaa_launches(g_ctx[0]));
    }
    f->file_bytes = ps[0].png_bytes;
    f->file_ms = ps[0].encode_ms + (with_map ? ps[1].encode_ms : 0.0);
    say_png(&ps[0], "16-bit PNG");
    if (!with_map) return 1;
    f->depth_file_bytes = ps[1].png_bytes;
    f->depth_ms = ndt_hip_depth_ms(g_ctx[0]);
    say_png(&ps[1], "16-bit depth PNG");
    say_map(f->range);
    return 1;
}

/* colour as the next frame's bytes of the animated PNG ndt_apng_begin opened (ndt_hip_render_apng_frame) */
static int frame_apng(const ndt_render_params *p, const ndt_frame_request *rq, ndt_frame *f)
{
    const int64_t cap = ndt_hip_apng_bound(p->width, p->height);
    const int K = rq->ssaa;
    ndt_apng_stats as;
    if (g_n_ctx > 1) {
        fprintf(stderr, "ndt_render_frame: the frames of an animated PNG meet one canvas on one GPU context, not on %d\n", g_n_ctx);
        return 0;
    }
    f->file = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
    if (!f->file) {
        fprintf(stderr, "ndt_render_frame: no animated PNG of %d x %d\n", p->width, p->height);
        return 0;
    }
    if (ndt_hip_render_apng_frame(g_ctx[0], p, K, f->file, cap, &as, NULL) != NDT_OK) return 0;
    if (K != 1) {
        f->ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
        say_ssaa(K, ndt_hip_ssaa_launches(g_ctx[0]));
    }
    f->file_bytes = as.bytes;
    f->file_ms = as.encode_ms;
    printf("animated PNG frame %d: %d x %d at %d,%d (%lld bytes) on GPU %d in %d launches\n", as.frame, as.w, as.h, as.x, as.y,
           (long long)as.bytes, ndt_hip_device(g_ctx[0]), as.launches);
    return 1;
}

/* colour as an OpenEXR file of half or float samples in linear light, the map of -z as its Z channel if asked (ndt_hip_render_exr,
 * ndt_hip_render_ssaa_exr; `ndt_hip --exr`); with exr_features the primary hit of every pixel as further channels of it
 * (ndt_hip_render_exr_features, ndt_hip_render_ssaa_exr_features; `--exr-aov`) */
static int frame_exr(const ndt_render_params *p, const ndt_frame_request *rq, ndt_frame *f, int dims)
{
    const int K = rq->ssaa, with_map = rq->map == NDT_MAP_EXR_Z;
    ndt_exr_params ep;
    ndt_exr_stats es;
    memset(&ep, 0, sizeof(ep));
    ep.pixel_type = rq->exr_pixel;
    const int features = rq->exr_features;
    if (features & ~(NDT_FEATURE_ID | NDT_FEATURE_POSITION | NDT_FEATURE_NORMAL)) {
        fprintf(stderr, "ndt_render_frame: exr_features %d: a mask of id 1, position 2, normal 4\n", features);
        return 0;
    }
    const int64_t cap = features ? ndt_hip_exr_features_bound(p->width, p->height, &ep, with_map, dims, features)
                                 : ndt_hip_exr_bound(p->width, p->height, &ep, with_map);
    if (g_n_ctx > 1) {
        /* (the rows of several contexts meet as 8-bit pixels or as doubles on the host: there is no float gather) */
        fprintf(stderr, "ndt_render_frame: an OpenEXR file is made by one GPU context, not by %d\n", g_n_ctx);
        return 0;
    }
    f->file = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
    if (!f->file) {
        fprintf(stderr, "ndt_render_frame: no OpenEXR file of %d x %d with pixel type %d\n", p->width, p->height, rq->exr_pixel);
        return 0;
    }
    if (features) {
        /* (no fallback: a frame the feature pass refuses -- -a, -n, anaglyph -- fails with the library's message) */
        if ((K != 1 ? ndt_hip_render_ssaa_exr_features(g_ctx[0], p, K, &ep, with_map, features, f->file, cap, &es, NULL)
                    : ndt_hip_render_exr_features(g_ctx[0], p, &ep, with_map, features, f->file, cap, &es, NULL)) != NDT_OK) return 0;
    } else if ((K != 1 ? ndt_hip_render_ssaa_exr(g_ctx[0], p, K, &ep, with_map, f->file, cap, &es, NULL)
                       : ndt_hip_render_exr(g_ctx[0], p, &ep, with_map, f->file, cap, &es, NULL)) != NDT_OK) return 0;
    if (K != 1) {
        f->ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
        say_ssaa(K, ndt_hip_ssaa_launches(g_ctx[0]));
    }
    f->file_bytes = es.file_bytes;
    f->file_ms = es.ms;
    printf("encoded EXR of %lld bytes on GPU %d in %d launches\n", (long long)es.file_bytes, ndt_hip_device(g_ctx[0]), es.launches);
    if (features) {
        f->feature_channels = (features & NDT_FEATURE_ID ? 1 : 0) + (features & NDT_FEATURE_POSITION ? dims : 0) + (features & NDT_FEATURE_NORMAL ? dims : 0);
        f->feature_launches = ndt_hip_features_launches(g_ctx[0]);
        printf("added %d feature channels on GPU %d in %d launches\n", f->feature_channels, ndt_hip_device(g_ctx[0]), f->feature_launches);
    }
    return 1;
}

/* `--denoise`: the frame denoised on the GPU behind the render (ndt_hip_render_denoised*): colour in doubles, as 8-bit RGBA, or as
 * a PNG, JPEG or OpenEXR file made there of the denoised doubles; one context, no map */
static ndt_denoise_params denoise_params_of(const ndt_frame_request *rq)
{
    ndt_denoise_params dp;
    memset(&dp, 0, sizeof(dp));
    dp.iterations = rq->denoise_iterations;
    dp.normal_power_log2 = rq->denoise_normal_power_log2;
    dp.sigma_colour = rq->denoise_sigma_colour;
    dp.sigma_plane = rq->denoise_sigma_plane;
    return dp;
}

static ndt_vdenoise_params vdenoise_params_of(const ndt_frame_request *rq)
{
    ndt_vdenoise_params vp;
    memset(&vp, 0, sizeof(vp));
    vp.iterations = rq->vdenoise_iterations;
    vp.normal_power_log2 = rq->vdenoise_normal_power_log2;
    vp.k_colour = rq->vdenoise_k_colour;
    vp.sigma_plane = rq->vdenoise_sigma_plane;
    return vp;
}

/* what a denoised frame does not go with, by name, before the scene is flattened or a device asked for (either filter) */
static int denoise_refused(const ndt_frame_request *rq)
{
    const char *why = NULL;
    const int variance = rq->vdenoise_iterations != 0;
    if (variance && rq->denoise_iterations != 0) why = "denoise_iterations: one stage stands between the render and the sink";
    else if (rq->aa_depth >= 0 && rq->aa_diff < 256) why = "recursive anti-aliasing (aa_depth >= 0): its pixels are averages of corner samples";
    else if (rq->stereo != 0) why = "a stereo mode: a stencil must not cross the seam between two eyes";
    else if (rq->ssaa != 1) why = "ssaa above 1: the guides are the plain frame's";
    else if (rq->map != NDT_MAP_NONE) why = "a depth map";
    else if (rq->exr_features) why = "exr_features";
    else if (rq->colour == NDT_COLOUR_PNG16 || rq->colour == NDT_COLOUR_APNG) why = "a 16-bit or an animated PNG";
    else if (g_want_ctx > 1) why = "a frame spread over several GPU contexts: a cyclic row shard has no neighbouring rows";
    if (why)
        fprintf(stderr, "ndt_render_frame: %s %d with %s: not built; there is no fallback\n", variance ? "vdenoise_iterations" : "denoise_iterations",
                variance ? rq->vdenoise_iterations : rq->denoise_iterations, why);
    return why != NULL;
}

static int frame_denoised(const ndt_render_params *p, const ndt_frame_request *rq, ndt_frame *f)
{
    const int width = p->width, height = p->height;
    const size_t n = (size_t)width * (size_t)height;
    const ndt_denoise_params dp = denoise_params_of(rq);
    const ndt_vdenoise_params vp = vdenoise_params_of(rq);
    const int variance = rq->vdenoise_iterations != 0;      /* the variance-guided filter: the same sinks through ndt_hip_render_vdenoised* */
    int ok;
    if (rq->colour == NDT_COLOUR_F64) {
        if (!(f->rgba = (double *)malloc(n * 4 * sizeof(double)))) return out_of_memory();
        ok = (variance ? ndt_hip_render_vdenoised(g_ctx[0], p, &vp, f->rgba, NULL) : ndt_hip_render_denoised(g_ctx[0], p, &dp, f->rgba, NULL)) == NDT_OK;
    } else if (rq->colour == NDT_COLOUR_RGBA8) {
        if (!(f->rgba8 = (unsigned char *)malloc(n * 4))) return out_of_memory();
        ok = (variance ? ndt_hip_render_vdenoised_rgba8(g_ctx[0], p, &vp, f->rgba8, NULL)
                       : ndt_hip_render_denoised_rgba8(g_ctx[0], p, &dp, f->rgba8, NULL)) == NDT_OK;
    } else if (rq->colour == NDT_COLOUR_EXR) {
        ndt_exr_params ep;
        ndt_exr_stats es;
        memset(&ep, 0, sizeof(ep));
        ep.pixel_type = rq->exr_pixel;
        const int64_t cap = ndt_hip_exr_bound(width, height, &ep, 0);
        f->file = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
        if (!f->file) {
            fprintf(stderr, "ndt_render_frame: no OpenEXR file of %d x %d with pixel type %d\n", width, height, rq->exr_pixel);
            return 0;
        }
        if (!(ok = (variance ? ndt_hip_render_vdenoised_exr(g_ctx[0], p, &vp, &ep, f->file, cap, &es, NULL)
                             : ndt_hip_render_denoised_exr(g_ctx[0], p, &dp, &ep, f->file, cap, &es, NULL)) == NDT_OK)) return 0;
        f->file_bytes = es.file_bytes;
        f->file_ms = es.ms;
        printf("encoded EXR of %lld bytes on GPU %d in %d launches\n", (long long)es.file_bytes, ndt_hip_device(g_ctx[0]), es.launches);
    } else {
        const int png = rq->colour == NDT_COLOUR_PNG;
        const ndt_jpeg_params jp = jpeg_params_of(rq->jpeg_quality, rq->jpeg_sampling);
        const int64_t cap = png ? ndt_hip_png_bound(width, height) : ndt_hip_jpeg_bound(width, height, &jp);
        ndt_png_stats ps;
        ndt_jpeg_stats js;
        f->file = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
        if (!f->file) {
            if (png) fprintf(stderr, "ndt_render_frame: no PNG of %d x %d\n", width, height);
            else fprintf(stderr, "ndt_render_frame: no JPEG of %d x %d at quality %d, sampling %d\n", width, height, jp.quality, jp.sampling);
            return 0;
        }
        if (variance)
            ok = (png ? ndt_hip_render_vdenoised_png(g_ctx[0], p, &vp, f->file, cap, &ps, NULL)
                      : ndt_hip_render_vdenoised_jpeg(g_ctx[0], p, &vp, &jp, f->file, cap, &js, NULL)) == NDT_OK;
        else
            ok = (png ? ndt_hip_render_denoised_png(g_ctx[0], p, &dp, f->file, cap, &ps, NULL)
                      : ndt_hip_render_denoised_jpeg(g_ctx[0], p, &dp, &jp, f->file, cap, &js, NULL)) == NDT_OK;
        if (!ok) return 0;
        f->file_bytes = png ? ps.png_bytes : js.jpeg_bytes;
        f->file_ms = png ? ps.encode_ms : js.encode_ms;
        if (png) say_png(&ps, "PNG");
        else say_jpeg(&js);
    }
    if (!ok) return 0;
    f->denoise_launches = ndt_hip_denoise_launches(g_ctx[0]);
    f->denoise_ms = ndt_hip_denoise_ms(g_ctx[0]);
    if (variance) printf("variance-guided denoise in %d iterations on GPU %d in %d launches\n", vp.iterations, ndt_hip_device(g_ctx[0]), f->denoise_launches);
    else printf("denoised in %d iterations on GPU %d in %d launches\n", dp.iterations, ndt_hip_device(g_ctx[0]), f->denoise_launches);
    return 1;
}

/* `--ao`: the frame's colour multiplied on the GPU by its ambient occlusion (ndt_hip_render_ao_shaded*): in doubles, as 8-bit RGBA,
 * as a PNG or JPEG file made there, or as the OpenEXR file with the channel AO, the feature channels and the map as Z
 * (ndt_hip_render_exr_ao); one context */
static ndt_ao_params ao_params_of(const ndt_frame_request *rq)
{
    ndt_ao_params ap;
    memset(&ap, 0, sizeof(ap));
    ap.samples = rq->ao_samples;
    ap.radius = rq->ao_radius;
    ap.seed = rq->ao_seed;
    ap.strength = rq->ao_strength;
    return ap;
}

/* what a frame with ambient occlusion does not go with, by name, before the scene is flattened or a device asked for */
static int ao_refused(const ndt_frame_request *rq)
{
    const char *why = NULL;
    if (rq->aa_depth >= 0 && rq->aa_diff < 256) why = "recursive anti-aliasing (aa_depth >= 0): its pixels are averages of corner samples";
    else if (rq->stereo == 3 || rq->stereo == 4) why = "anaglyph or frame-packed stereo: no single primary ray a pixel";
    else if (rq->ssaa != 1) why = "ssaa above 1: the occlusion is the plain frame's";
    else if (rq->map != NDT_MAP_NONE && rq->map != NDT_MAP_EXR_Z) why = "a depth map that is not the Z channel of the OpenEXR file";
    else if (rq->colour == NDT_COLOUR_PNG16 || rq->colour == NDT_COLOUR_APNG) why = "a 16-bit or an animated PNG";
    else if (rq->denoise_iterations != 0) why = "denoise_iterations: one stage stands between the render and the sink";
    else if (rq->vdenoise_iterations != 0) why = "vdenoise_iterations: one stage stands between the render and the sink";
    else if (g_want_ctx > 1) why = "a frame spread over several GPU contexts";
    else if (rq->ao_samples < 1 || rq->ao_samples > 256) why = "a sample count outside 1 .. 256";
    if (why) fprintf(stderr, "ndt_render_frame: ao_samples %d with %s: not built; there is no fallback\n", rq->ao_samples, why);
    return why != NULL;
}

static int frame_ao(const ndt_render_params *p, const ndt_frame_request *rq, ndt_frame *f, int dims)
{
    const int width = p->width, height = p->height;
    const size_t n = (size_t)width * (size_t)height;
    const ndt_ao_params ap = ao_params_of(rq);
    int ok;
    if (rq->colour == NDT_COLOUR_F64) {
        if (!(f->rgba = (double *)malloc(n * 4 * sizeof(double)))) return out_of_memory();
        ok = ndt_hip_render_ao_shaded(g_ctx[0], p, &ap, f->rgba, NULL, NULL) == NDT_OK;
    } else if (rq->colour == NDT_COLOUR_RGBA8) {
        if (!(f->rgba8 = (unsigned char *)malloc(n * 4))) return out_of_memory();
        ok = ndt_hip_render_ao_shaded_rgba8(g_ctx[0], p, &ap, f->rgba8, NULL) == NDT_OK;
    } else if (rq->colour == NDT_COLOUR_EXR) {
        const int with_map = rq->map == NDT_MAP_EXR_Z, features = rq->exr_features;
        ndt_exr_params ep;
        ndt_exr_stats es;
        memset(&ep, 0, sizeof(ep));
        ep.pixel_type = rq->exr_pixel;
        const int64_t cap = ndt_hip_exr_ao_bound(width, height, &ep, with_map, dims, features);
        f->file = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
        if (!f->file) {
            fprintf(stderr, "ndt_render_frame: no OpenEXR file of %d x %d with pixel type %d and exr_features %d\n", width, height, rq->exr_pixel, features);
            return 0;
        }
        if (!(ok = ndt_hip_render_exr_ao(g_ctx[0], p, &ep, with_map, features, &ap, f->file, cap, &es, NULL) == NDT_OK)) return 0;
        f->file_bytes = es.file_bytes;
        f->file_ms = es.ms;
        printf("encoded EXR of %lld bytes on GPU %d in %d launches\n", (long long)es.file_bytes, ndt_hip_device(g_ctx[0]), es.launches);
        if (features) {
            f->feature_channels = (features & NDT_FEATURE_ID ? 1 : 0) + (features & NDT_FEATURE_POSITION ? dims : 0) + (features & NDT_FEATURE_NORMAL ? dims : 0);
            f->feature_launches = ndt_hip_features_launches(g_ctx[0]);
            printf("added %d feature channels on GPU %d in %d launches\n", f->feature_channels, ndt_hip_device(g_ctx[0]), f->feature_launches);
        }
    } else {
        const int png = rq->colour == NDT_COLOUR_PNG;
        const ndt_jpeg_params jp = jpeg_params_of(rq->jpeg_quality, rq->jpeg_sampling);
        const int64_t cap = png ? ndt_hip_png_bound(width, height) : ndt_hip_jpeg_bound(width, height, &jp);
        ndt_png_stats ps;
        ndt_jpeg_stats js;
        f->file = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
        if (!f->file) {
            if (png) fprintf(stderr, "ndt_render_frame: no PNG of %d x %d\n", width, height);
            else fprintf(stderr, "ndt_render_frame: no JPEG of %d x %d at quality %d, sampling %d\n", width, height, jp.quality, jp.sampling);
            return 0;
        }
        ok = (png ? ndt_hip_render_ao_shaded_png(g_ctx[0], p, &ap, f->file, cap, &ps, NULL)
                  : ndt_hip_render_ao_shaded_jpeg(g_ctx[0], p, &ap, &jp, f->file, cap, &js, NULL)) == NDT_OK;
        if (!ok) return 0;
        f->file_bytes = png ? ps.png_bytes : js.jpeg_bytes;
        f->file_ms = png ? ps.encode_ms : js.encode_ms;
        if (png) say_png(&ps, "PNG");
        else say_jpeg(&js);
    }
    if (!ok) return 0;
    f->ao_launches = ndt_hip_ao_launches(g_ctx[0]);
    f->ao_ms = ndt_hip_ao_ms(g_ctx[0]);
    printf("ambient occlusion of %d samples on GPU %d in %d launches\n", ap.samples, ndt_hip_device(g_ctx[0]), f->ao_launches);
    return 1;
}

/* the maps each colour kind comes with (bit m: ndt_map_kind m): the pairs a device call serves */
#define MAP_BIT(m) (1u << (m))
static const struct { const char *name; unsigned maps; } colour_kinds[] = {
    { "doubles", MAP_BIT(NDT_MAP_NONE) | MAP_BIT(NDT_MAP_F64) },
    { "8-bit RGBA", MAP_BIT(NDT_MAP_NONE) | MAP_BIT(NDT_MAP_DEPTH8) },
    { "PNG file", MAP_BIT(NDT_MAP_NONE) | MAP_BIT(NDT_MAP_DEPTH8) | MAP_BIT(NDT_MAP_PNG) },
    { "JPEG file", MAP_BIT(NDT_MAP_NONE) },
    { "16-bit PNG file", MAP_BIT(NDT_MAP_NONE) | MAP_BIT(NDT_MAP_PNG16) },
    { "animated PNG frame", MAP_BIT(NDT_MAP_NONE) },
    { "OpenEXR file", MAP_BIT(NDT_MAP_NONE) | MAP_BIT(NDT_MAP_EXR_Z) },
};
static const char *const map_kinds[] = { "none", "doubles", "8-bit grey finished on the GPU", "PNG file", "16-bit PNG file",
                                         "the Z channel of the OpenEXR file" };

int ndt_render_frame(scene *scn, const ndt_frame_request *rq, ndt_frame *f)
{
    char err[256];
    ndt_flat_builder fb;
    /* NDT_HOST_TIMING=1: where a frame's host time goes (stderr) */
    /* (read per call: a static written by concurrent host threads -- ndt_hip -j K -- would be a data race) */
    const int timing = getenv("NDT_HOST_TIMING") != NULL;
    struct timespec ts0, ts1, ts2, ts3;
    memset(f, 0, sizeof(*f));
    if ((unsigned)rq->colour > NDT_COLOUR_EXR || (unsigned)rq->map > NDT_MAP_EXR_Z || !(colour_kinds[rq->colour].maps & MAP_BIT(rq->map))) {
        fprintf(stderr, "ndt_render_frame: no device call brings colour (%s) and map (%s) of one frame\n",
                (unsigned)rq->colour > NDT_COLOUR_EXR ? "unknown" : colour_kinds[rq->colour].name,
                (unsigned)rq->map > NDT_MAP_EXR_Z ? "unknown" : map_kinds[rq->map]);
        return 0;
    }
    if (rq->exr_features && rq->colour != NDT_COLOUR_EXR) {
        fprintf(stderr, "ndt_render_frame: exr_features are channels of the OpenEXR file: colour (%s) has none\n", colour_kinds[rq->colour].name);
        return 0;
    }
    if ((rq->denoise_iterations != 0 || rq->vdenoise_iterations != 0) && denoise_refused(rq)) return 0;
    if (rq->sample_cap < 0) {
        fprintf(stderr, "ndt_render_frame: sample_cap %d: 0 for no cap, or the most samples a pixel takes\n", rq->sample_cap);
        return 0;
    }
    if (rq->ao_samples != 0 && ao_refused(rq)) return 0;
    /* 1. the scene: flattened, uploaded to every context of the thread (the pthread fan-out of ndt.c:949-975 is the GPU's job now;
     * `threads` fits the scene's bounding spheres in parallel) */
    if (timing) clock_gettime(CLOCK_MONOTONIC, &ts0);
    ndt_fit_stats fit;
    ndt_kd_stats kds;
    if (ndt_flatten_scene_gpu(scn, &fb, err, sizeof(err), rq->threads, g_fit_on_gpu, g_kd_on_gpu, &fit, &kds) != 0) {
        fprintf(stderr, "ndt_render_image: %s\n", err);
        ndt_flat_builder_free(&fb);
        return 0;
    }
    if (timing) clock_gettime(CLOCK_MONOTONIC, &ts1);
    int ok = have_contexts();
    for (int k = 0; ok && k < g_n_ctx; ++k)
        if (ndt_hip_upload_scene(g_ctx[k], &fb.fs) != NDT_OK) ok = 0;
    if (ok && rq->sample_cap != g_sample_cap) {     /* (a thread that never asks for a cap leaves its contexts as they were created) */
        for (int k = 0; ok && k < g_n_ctx; ++k)
            if (ndt_hip_set_option(g_ctx[k], "sample_cap", rq->sample_cap) != NDT_OK) ok = 0;
        if (ok) g_sample_cap = rq->sample_cap;
    }
    if (timing) clock_gettime(CLOCK_MONOTONIC, &ts2);
    const int map8 = rq->map == NDT_MAP_DEPTH8 || rq->map == NDT_MAP_PNG;
    if (ok) {
        ndt_render_params p;
        memset(&p, 0, sizeof(p));
        p.width = rq->width; p.height = rq->height; p.max_optic_depth = rq->max_optic_depth; p.samples = rq->samples > 1 ? rq->samples : 1;
        p.row_begin = 0; p.row_step = 1; p.specular = rq->specular;
        p.stereo = rq->stereo;
        if (rq->aa_depth >= 0 && rq->aa_diff < 256) {       /* ndt.c:1040: otherwise the first pass is the image */
            p.recursive_aa = 1;
            p.aa_diff = rq->aa_diff;
            p.aa_depth = rq->aa_depth;
        }
        /* 2. and 3. colour and map in the forms asked for: one device call makes both, so the routine is chosen by the pair */
        if (rq->denoise_iterations != 0 || rq->vdenoise_iterations != 0) ok = frame_denoised(&p, rq, f);
        else if (rq->ao_samples != 0) ok = frame_ao(&p, rq, f, fb.fs.dims);
        else if (rq->colour == NDT_COLOUR_EXR) ok = frame_exr(&p, rq, f, fb.fs.dims);
        else if (rq->colour == NDT_COLOUR_APNG) ok = frame_apng(&p, rq, f);
        else if (rq->colour == NDT_COLOUR_PNG16) ok = frame_png16(&p, rq, f);
        else if (map8) ok = frame_beside_map8(&p, rq, f);
        else if (rq->colour == NDT_COLOUR_PNG || rq->colour == NDT_COLOUR_JPEG) ok = frame_file(&p, rq, f);
        else ok = frame_pixels(&p, rq, f);
        /* 4. what is left to report (each routine has said what the device did, in the order it did it) */
        if (ok && g_n_ctx > 1 && !g_paths_said) {
            /* once per thread: how every context's rows reached the frame (an N-GPU run is diagnosable from its log) */
            static const char *const names[] = { "no rows", "same device", "peer stores", "staged copy" };
            g_paths_said = 1;
            fprintf(stderr, "ndt_render_image: one frame over %d contexts:", g_n_ctx);
            for (int k = 0; k < g_n_ctx; ++k) {
                const int path = ndt_hip_multi_path_taken(g_ctx[k]);
                fprintf(stderr, " [%d] GPU %d %s%s", k, ndt_hip_device(g_ctx[k]), names[path >= 0 && path <= 3 ? path : 0], k + 1 < g_n_ctx ? "," : "\n");
            }
        }
    }
    if (!ok) fprintf(stderr, "ndt_render_image: %s\n", ndt_hip_last_error());
    if (timing) {
        clock_gettime(CLOCK_MONOTONIC, &ts3);
#define NDT_MS(a, b) (((b).tv_sec - (a).tv_sec) * 1e3 + ((b).tv_nsec - (a).tv_nsec) * 1e-6)
        /* the first figure split: the sphere fits (on the GPU: gathering the bounding points / the fit calls) and the rest */
        /* ... and of the rest the kd-tree build on its own, whoever made it */
        char share[240], tree[64];
        if (g_kd_on_gpu) snprintf(tree, sizeof(tree), "kd-tree on GPU %.2f in %d launches", kds.build_ms, g_kd_launches);
        else snprintf(tree, sizeof(tree), "kd-tree %.2f", kds.build_ms);
        if (g_fit_on_gpu)
            snprintf(share, sizeof(share), "gpu fits: points gathered %.2f + fit %.2f, %s, rest %.2f", fit.gather_ms, fit.fit_ms, tree,
                     NDT_MS(ts0, ts1) - fit.gather_ms - fit.fit_ms - kds.build_ms);
        else
            snprintf(share, sizeof(share), "host fits %.2f, %s, rest %.2f", fit.fit_ms, tree, NDT_MS(ts0, ts1) - fit.fit_ms - kds.build_ms);
        char what[200];     /* one fprintf a line: the workers of -j K share stderr */
        if (map8 && ok)
            snprintf(what, sizeof(what), "8-bit image and depth map to host %.2f ms (depth map finished on the GPU %.2f%s)", NDT_MS(ts2, ts3),
                     f->depth_ms, rq->colour == NDT_COLOUR_PNG ? ", image files made there" : "");
        else if (rq->colour == NDT_COLOUR_APNG && ok)
            snprintf(what, sizeof(what), "the frame's bytes of the animated PNG to host %.2f ms (plan and file bytes on the GPU %.2f)",
                     NDT_MS(ts2, ts3), f->file_ms);
        else if (rq->colour >= NDT_COLOUR_PNG && ok)
            snprintf(what, sizeof(what), "image file to host %.2f ms (image file on the GPU %.2f)", NDT_MS(ts2, ts3), f->file_ms);
        else
            snprintf(what, sizeof(what), "image to host %.2f ms", NDT_MS(ts2, ts3));
        fprintf(stderr, "ndt_render_image: bounds + kd-tree + flatten %.2f ms (%s), upload %.2f ms, render + %s\n", NDT_MS(ts0, ts1), share,
                NDT_MS(ts1, ts2), what);
        if (rq->denoise_iterations != 0 && ok)
            fprintf(stderr, "ndt_render_image: behind the render, the denoiser's %d iterations on the GPU %.2f ms\n", rq->denoise_iterations, f->denoise_ms);
        if (rq->ao_samples != 0 && ok)
            fprintf(stderr, "ndt_render_image: behind the render, the ambient occlusion of %d samples on the GPU %.2f ms\n", rq->ao_samples, f->ao_ms);
        if (rq->ssaa != 1 && ok)
            fprintf(stderr, "ndt_render_image: of the render, supersampling %dx%d: the folds on the GPU %.2f ms\n", rq->ssaa, rq->ssaa, f->ssaa_ms);
    }
    ndt_flat_builder_free(&fb);
    if (!ok) ndt_frame_free(f);
    return ok;
}
