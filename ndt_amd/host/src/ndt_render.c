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

static void drop_contexts(void)
{
    for (int k = 0; k < g_n_ctx; ++k) ndt_hip_destroy(g_ctx[k]);
    g_n_ctx = 0;
    g_paths_said = 0;
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

/* render_image with the reference's `-a diff,depth` (recursive_aa, ndt.c:44, 1039-1087); aa_depth < 0 = plain */
int ndt_render_image_aa(scene *scn, int width, int height, int threads, int aa_diff, int aa_depth, int max_optic_depth,
                        double *rgba)
{
    return ndt_render_image_full(scn, width, height, 1, threads, aa_diff, aa_depth, 0, 1, max_optic_depth, rgba, NULL);
}

/* ---- the frame's PNG file made on the GPU (ndt_hip_render_png / ndt_hip_encode_png) */
#define NDT_HOST_IMAGE_PNG 100              /* render_any's `format` beside ndt_image_format; `out` is a png_out */
typedef struct { unsigned char **png; long long *bytes; } png_out;
static __thread double g_png_ms = 0.0;

double ndt_render_png_encode_ms(void) { return g_png_ms; }

static void say_png(const ndt_png_stats *ps)
{
    g_png_ms = ps->encode_ms;
    printf("compressed PNG of %lld bytes on GPU %d in %d launches\n", (long long)ps->png_bytes, ndt_hip_device(g_ctx[0]), ps->launches);
}

int ndt_encode_image_png(const unsigned char *rgba8, int width, int height, unsigned char **png, long long *png_bytes)
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
    say_png(&ps);
    *png = buf;
    *png_bytes = ps.png_bytes;
    return 1;
}

/* ---- the frame's JPEG file made on the GPU (ndt_hip_render_jpeg / ndt_hip_encode_jpeg) */
#define NDT_HOST_IMAGE_JPEG 102             /* render_any's `format`; `out` is a jpeg_out */
typedef struct { unsigned char **jpg; long long *bytes; ndt_jpeg_params jp; } jpeg_out;
static __thread double g_jpeg_ms = 0.0;

double ndt_render_jpeg_encode_ms(void) { return g_jpeg_ms; }

static void say_jpeg(const ndt_jpeg_stats *js)
{
    g_jpeg_ms = js->encode_ms;
    printf("encoded JPEG of %lld bytes on GPU %d in %d launches\n", (long long)js->jpeg_bytes, ndt_hip_device(g_ctx[0]), js->launches);
}

static ndt_jpeg_params jpeg_params_of(int quality, int sampling)
{
    ndt_jpeg_params jp;
    memset(&jp, 0, sizeof(jp));
    jp.quality = quality;
    jp.sampling = sampling;
    return jp;
}

int ndt_encode_image_jpeg(const unsigned char *rgba8, int width, int height, int quality, int sampling, unsigned char **jpg, long long *jpg_bytes)
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
    return 1;
}

/* ---- the depth map of -z finished on the GPU (ndt_hip_render_rgba8_depth / ndt_hip_render_png_depth) */
#define NDT_HOST_IMAGE_DEPTH8 101           /* render_any's `format`; `out` is a depth_out */
typedef struct { ndt_depth_frame *frame; int want_png, want_depth_png; } depth_out;
static __thread double g_depth_ms = 0.0;

double ndt_render_depth_finish_ms(void) { return g_depth_ms; }

void ndt_depth_frame_free(ndt_depth_frame *f)
{
    free(f->rgba8);
    free(f->depth8);
    free(f->png);
    free(f->depth_png);
    memset(f, 0, sizeof(*f));
}

static int render_depth8(const ndt_render_params *p, depth_out *d)
{
    ndt_depth_frame *f = d->frame;
    const size_t bytes = (size_t)p->width * (size_t)p->height * 4;
    int rc;
    if (d->want_png) {
        const int64_t cap = ndt_hip_png_bound(p->width, p->height);
        ndt_png_stats ps[2];
        if (cap < 0) {
            fprintf(stderr, "ndt_render_image_depth8: no PNG of %d x %d\n", p->width, p->height);
            return 0;
        }
        f->png = (unsigned char *)malloc((size_t)cap);
        if (d->want_depth_png) f->depth_png = (unsigned char *)malloc((size_t)cap);
        else f->depth8 = (unsigned char *)malloc(bytes);
        if (!f->png || !(d->want_depth_png ? f->depth_png : f->depth8)) return 0;
        rc = ndt_hip_render_png_depth(g_ctx[0], p, f->png, cap, f->depth_png, cap, f->depth8, ps, f->range, NULL);
        if (rc != NDT_OK) return 0;
        f->png_bytes = ps[0].png_bytes;
        f->depth_png_bytes = ps[1].png_bytes;
        g_png_ms = ps[0].encode_ms + ps[1].encode_ms;
        printf("compressed PNG of %lld bytes on GPU %d in %d launches\n", (long long)ps[0].png_bytes, ndt_hip_device(g_ctx[0]), ps[0].launches);
        if (d->want_depth_png)
            printf("compressed depth PNG of %lld bytes on GPU %d in %d launches\n", (long long)ps[1].png_bytes, ndt_hip_device(g_ctx[0]), ps[1].launches);
    } else {
        f->rgba8 = (unsigned char *)malloc(bytes);
        f->depth8 = (unsigned char *)malloc(bytes);
        if (!f->rgba8 || !f->depth8) return 0;
        rc = ndt_hip_render_rgba8_depth(g_ctx[0], p, f->rgba8, f->depth8, f->range, NULL);
        if (rc != NDT_OK) return 0;
    }
    g_depth_ms = ndt_hip_depth_ms(g_ctx[0]);
    printf("finished depth map [%.17g, %.17g] on GPU %d in %d launches\n", f->range[0], f->range[1], ndt_hip_device(g_ctx[0]),
           ndt_hip_depth_launches(g_ctx[0]));
    return 1;
}

/* ---- the frame supersampled K x K on the GPU (ndt_hip_render_ssaa*; `ndt_hip --ssaa K`) */
static __thread double g_ssaa_ms = 0.0;

double ndt_render_ssaa_fold_ms(void) { return g_ssaa_ms; }

/* the doubles (format NDT_IMAGE_F64) or the bytes (NDT_IMAGE_RGBA8) of the ssaa frame in host memory: from the one context, or
 * from several, each of which renders and folds its own cyclic row shard, context after context */
static int ssaa_image(const ndt_render_params *p, int K, int format, void *out, int *launches)
{
    const size_t px = format == NDT_IMAGE_F64 ? 4 * sizeof(double) : 4;
    *launches = 0;
    g_ssaa_ms = 0.0;
    if (g_n_ctx == 1) {
        const int rc = format == NDT_IMAGE_F64 ? ndt_hip_render_ssaa(g_ctx[0], p, K, (double *)out, NULL, NULL)
                                               : ndt_hip_render_ssaa_rgba8(g_ctx[0], p, K, (unsigned char *)out, NULL);
        *launches = ndt_hip_ssaa_launches(g_ctx[0]);
        g_ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
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
        g_ssaa_ms += ndt_hip_ssaa_ms(g_ctx[k]);
    }
    free(part);
    return ok;
}

/* every format of render_any for an ssaa frame */
static int render_ssaa_any(const ndt_render_params *p, int K, int format, void *out, double *depth)
{
    const int width = p->width, height = p->height;
    int ok = 0, launches = 0;
    if (format == NDT_HOST_IMAGE_PNG || format == NDT_HOST_IMAGE_JPEG) {
        const int png = format == NDT_HOST_IMAGE_PNG;
        png_out *po = (png_out *)out;
        jpeg_out *jo = (jpeg_out *)out;
        const int64_t cap = png ? ndt_hip_png_bound(width, height) : ndt_hip_jpeg_bound(width, height, &jo->jp);
        ndt_png_stats ps;
        ndt_jpeg_stats js;
        unsigned char *buf = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
        if (!buf) {
            fprintf(stderr, "ndt_render_image_ssaa: no %s of %d x %d\n", png ? "PNG" : "JPEG", width, height);
            return 0;
        }
        if (g_n_ctx == 1) {
            ok = (png ? ndt_hip_render_ssaa_png(g_ctx[0], p, K, buf, cap, &ps, NULL)
                      : ndt_hip_render_ssaa_jpeg(g_ctx[0], p, K, &jo->jp, buf, cap, &js, NULL)) == NDT_OK;
            launches = ndt_hip_ssaa_launches(g_ctx[0]);
            g_ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
        } else {
            /* rows from several contexts: gathered into host memory, encoded from there on the first context */
            unsigned char *rgba8 = (unsigned char *)malloc((size_t)width * height * 4);
            ok = rgba8 && ssaa_image(p, K, NDT_IMAGE_RGBA8, rgba8, &launches) &&
                 (png ? ndt_hip_encode_png(g_ctx[0], rgba8, width, height, buf, cap, &ps)
                      : ndt_hip_encode_jpeg(g_ctx[0], rgba8, width, height, &jo->jp, buf, cap, &js)) == NDT_OK;
            free(rgba8);
        }
        if (!ok) free(buf);
        else if (png) {
            say_png(&ps);
            *po->png = buf;
            *po->bytes = ps.png_bytes;
        } else {
            say_jpeg(&js);
            *jo->jpg = buf;
            *jo->bytes = js.jpeg_bytes;
        }
    } else if (format == NDT_HOST_IMAGE_DEPTH8) {
        /* (one context, like every frame with a map) the two 8-bit images come back; files are encoded from them */
        depth_out *d = (depth_out *)out;
        ndt_depth_frame *f = d->frame;
        const size_t bytes = (size_t)width * (size_t)height * 4;
        f->rgba8 = (unsigned char *)malloc(bytes);
        f->depth8 = (unsigned char *)malloc(bytes);
        ok = f->rgba8 && f->depth8 && ndt_hip_render_ssaa_rgba8_depth(g_ctx[0], p, K, f->rgba8, f->depth8, f->range, NULL) == NDT_OK;
        launches = ndt_hip_ssaa_launches(g_ctx[0]);
        g_ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
        if (ok) {
            g_depth_ms = ndt_hip_depth_ms(g_ctx[0]);
            printf("finished depth map [%.17g, %.17g] on GPU %d in %d launches\n", f->range[0], f->range[1], ndt_hip_device(g_ctx[0]),
                   ndt_hip_depth_launches(g_ctx[0]));
        }
        if (ok && d->want_png) {
            ok = ndt_encode_image_png(f->rgba8, width, height, &f->png, &f->png_bytes);
            free(f->rgba8);
            f->rgba8 = NULL;
            if (ok && d->want_depth_png) {
                const double image_ms = g_png_ms;
                ok = ndt_encode_image_png(f->depth8, width, height, &f->depth_png, &f->depth_png_bytes);
                g_png_ms += image_ms;
                free(f->depth8);
                f->depth8 = NULL;
            }
        }
    } else if (depth) {     /* the depth map comes from the one-context call (a map is not split over devices) */
        ok = format == NDT_IMAGE_F64 && ndt_hip_render_ssaa(g_ctx[0], p, K, (double *)out, depth, NULL) == NDT_OK;
        launches = ndt_hip_ssaa_launches(g_ctx[0]);
        g_ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
    } else
        ok = ssaa_image(p, K, format, out, &launches);
    if (ok) printf("supersampled %dx%d on GPU %d in %d launches\n", K, K, ndt_hip_device(g_ctx[0]), launches);
    return ok;
}

/* ---- the frame's files at 16 bits a sample (ndt_hip_render_png16*, ndt_hip_render_ssaa_png16*; `ndt_hip --png16`) */
#define NDT_HOST_IMAGE_PNG16 103            /* render_any's `format`; `out` is a png_out */
#define NDT_HOST_IMAGE_PNG16_DEPTH 104      /* ... `out` is an ndt_depth_frame: png and depth_png arrive */

static int render_png16(const ndt_render_params *p, int K, int format, void *out)
{
    const int width = p->width, height = p->height, with_map = format == NDT_HOST_IMAGE_PNG16_DEPTH;
    const int64_t cap = ndt_hip_png16_bound(width, height, 4), depth_cap = ndt_hip_png16_bound(width, height, 1);
    ndt_png_stats ps[2];
    double range[2] = { 0.0, 0.0 };
    if (g_n_ctx > 1) {
        /* (the rows of several contexts meet as 8-bit pixels or as doubles on the host: there is no 16-bit gather) */
        fprintf(stderr, "ndt_render_image_png16: a 16-bit PNG is made by one GPU context, not by %d\n", g_n_ctx);
        return 0;
    }
    if (cap < 0 || depth_cap < 0) {
        fprintf(stderr, "ndt_render_image_png16: no 16-bit PNG of %d x %d\n", width, height);
        return 0;
    }
    unsigned char *buf = (unsigned char *)malloc((size_t)cap), *dbuf = with_map ? (unsigned char *)malloc((size_t)depth_cap) : NULL;
    int ok = buf && (dbuf || !with_map);
    if (ok && with_map)
        ok = (K != 1 ? ndt_hip_render_ssaa_png16_depth(g_ctx[0], p, K, buf, cap, dbuf, depth_cap, ps, range, NULL)
                     : ndt_hip_render_png16_depth(g_ctx[0], p, buf, cap, dbuf, depth_cap, ps, range, NULL)) == NDT_OK;
    else if (ok)
        ok = (K != 1 ? ndt_hip_render_ssaa_png16(g_ctx[0], p, K, buf, cap, ps, NULL) : ndt_hip_render_png16(g_ctx[0], p, buf, cap, ps, NULL)) == NDT_OK;
    if (!ok) {
        free(buf);
        free(dbuf);
        return 0;
    }
    if (K != 1) {
        g_ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
        printf("supersampled %dx%d on GPU %d in %d launches\n", K, K, ndt_hip_device(g_ctx[0]), ndt_hip_ssaa_launches(g_ctx[0]));
    }
    g_png_ms = ps[0].encode_ms + (with_map ? ps[1].encode_ms : 0.0);
    printf("compressed 16-bit PNG of %lld bytes on GPU %d in %d launches\n", (long long)ps[0].png_bytes, ndt_hip_device(g_ctx[0]), ps[0].launches);
    if (!with_map) {
        png_out *po = (png_out *)out;
        *po->png = buf;
        *po->bytes = ps[0].png_bytes;
        return 1;
    }
    ndt_depth_frame *f = (ndt_depth_frame *)out;
    f->png = buf;
    f->png_bytes = ps[0].png_bytes;
    f->depth_png = dbuf;
    f->depth_png_bytes = ps[1].png_bytes;
    f->range[0] = range[0];
    f->range[1] = range[1];
    g_depth_ms = ndt_hip_depth_ms(g_ctx[0]);
    printf("compressed 16-bit depth PNG of %lld bytes on GPU %d in %d launches\n", (long long)ps[1].png_bytes, ndt_hip_device(g_ctx[0]), ps[1].launches);
    printf("finished depth map [%.17g, %.17g] on GPU %d in %d launches\n", f->range[0], f->range[1], ndt_hip_device(g_ctx[0]),
           ndt_hip_depth_launches(g_ctx[0]));
    return 1;
}

/* ---- the run's frames as one animated PNG (ndt_hip_apng_*, ndt_hip_render_apng_frame; `ndt_hip --apng`) */
#define NDT_HOST_IMAGE_APNG 105             /* render_any's `format`; `out` is a png_out: the bytes to append */
static __thread double g_apng_ms = 0.0;

double ndt_render_apng_encode_ms(void) { return g_apng_ms; }

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

static int render_apng(const ndt_render_params *p, int K, png_out *po)
{
    const int64_t cap = ndt_hip_apng_bound(p->width, p->height);
    ndt_apng_stats as;
    if (g_n_ctx > 1) {
        fprintf(stderr, "ndt_render_image_apng_frame: the frames of an animated PNG meet one canvas on one GPU context, not on %d\n", g_n_ctx);
        return 0;
    }
    unsigned char *buf = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
    if (!buf) {
        fprintf(stderr, "ndt_render_image_apng_frame: no animated PNG of %d x %d\n", p->width, p->height);
        return 0;
    }
    if (ndt_hip_render_apng_frame(g_ctx[0], p, K, buf, cap, &as, NULL) != NDT_OK) {
        free(buf);
        return 0;
    }
    if (K != 1) {
        g_ssaa_ms = ndt_hip_ssaa_ms(g_ctx[0]);
        printf("supersampled %dx%d on GPU %d in %d launches\n", K, K, ndt_hip_device(g_ctx[0]), ndt_hip_ssaa_launches(g_ctx[0]));
    }
    g_apng_ms = as.encode_ms;
    printf("animated PNG frame %d: %d x %d at %d,%d (%lld bytes) on GPU %d in %d launches\n", as.frame, as.w, as.h, as.x, as.y,
           (long long)as.bytes, ndt_hip_device(g_ctx[0]), as.launches);
    *po->png = buf;
    *po->bytes = as.bytes;
    return 1;
}

static int render_any(scene *scn, int width, int height, int samples, int aa_diff, int aa_depth, int stereo, int specular,
                      int max_optic_depth, int format, void *out, double *depth, int threads, int ssaa)
{
    char err[256];
    ndt_flat_builder fb;
    /* NDT_HOST_TIMING=1: where a frame's host time goes (stderr) */
    /* (read per call: a static written by concurrent host threads -- ndt_hip -j K -- would be a data race) */
    const int timing = getenv("NDT_HOST_TIMING") != NULL;
    struct timespec ts0, ts1, ts2, ts3;
    if (timing) clock_gettime(CLOCK_MONOTONIC, &ts0);
    ndt_fit_stats fit;
    ndt_kd_stats kds;
    if (ndt_flatten_scene_gpu(scn, &fb, err, sizeof(err), threads, g_fit_on_gpu, g_kd_on_gpu, &fit, &kds) != 0) {
        fprintf(stderr, "ndt_render_image: %s\n", err);
        ndt_flat_builder_free(&fb);
        return 0;
    }
    if (timing) clock_gettime(CLOCK_MONOTONIC, &ts1);
    int ok = have_contexts();
    for (int k = 0; ok && k < g_n_ctx; ++k)
        if (ndt_hip_upload_scene(g_ctx[k], &fb.fs) != NDT_OK) ok = 0;
    if (timing) clock_gettime(CLOCK_MONOTONIC, &ts2);
    if (ok) {
        ndt_render_params p;
        memset(&p, 0, sizeof(p));
        p.width = width; p.height = height; p.max_optic_depth = max_optic_depth; p.samples = samples > 1 ? samples : 1;
        p.row_begin = 0; p.row_step = 1; p.specular = specular;
        p.stereo = stereo;
        if (aa_depth >= 0 && aa_diff < 256) {       /* ndt.c:1040: otherwise the first pass is the image */
            p.recursive_aa = 1;
            p.aa_diff = aa_diff;
            p.aa_depth = aa_depth;
        }
        if (format == NDT_HOST_IMAGE_APNG) {
            ok = render_apng(&p, ssaa, (png_out *)out);
        } else if (format == NDT_HOST_IMAGE_PNG16 || format == NDT_HOST_IMAGE_PNG16_DEPTH) {
            ok = render_png16(&p, ssaa, format, out);
        } else if (ssaa != 1) {        /* (0, 9, ... reach the library, which says what is wrong with them) */
            ok = render_ssaa_any(&p, ssaa, format, out, depth);
        } else if (format == NDT_HOST_IMAGE_PNG) {
            png_out *po = (png_out *)out;
            const int64_t cap = ndt_hip_png_bound(width, height);
            ndt_png_stats ps;
            unsigned char *buf = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
            if (!buf) {
                fprintf(stderr, "ndt_render_image_png: no PNG of %d x %d\n", width, height);
                ok = 0;
            } else if (g_n_ctx == 1) {
                ok = ndt_hip_render_png(g_ctx[0], &p, buf, cap, &ps, NULL) == NDT_OK;
            } else {
                /* rows from several contexts: gathered into host memory, encoded from there on the first context */
                unsigned char *rgba8 = (unsigned char *)malloc((size_t)width * height * 4);
                ok = rgba8 && ndt_hip_render_multi(g_ctx, g_n_ctx, &p, NDT_IMAGE_RGBA8, rgba8, NULL) == NDT_OK &&
                     ndt_hip_encode_png(g_ctx[0], rgba8, width, height, buf, cap, &ps) == NDT_OK;
                free(rgba8);
            }
            if (ok) {
                say_png(&ps);
                *po->png = buf;
                *po->bytes = ps.png_bytes;
            } else free(buf);
        } else if (format == NDT_HOST_IMAGE_JPEG) {
            jpeg_out *jo = (jpeg_out *)out;
            const int64_t cap = ndt_hip_jpeg_bound(width, height, &jo->jp);
            ndt_jpeg_stats js;
            unsigned char *buf = cap > 0 ? (unsigned char *)malloc((size_t)cap) : NULL;
            if (!buf) {
                fprintf(stderr, "ndt_render_image_jpeg: no JPEG of %d x %d at quality %d, sampling %d\n", width, height, jo->jp.quality, jo->jp.sampling);
                ok = 0;
            } else if (g_n_ctx == 1) {
                ok = ndt_hip_render_jpeg(g_ctx[0], &p, &jo->jp, buf, cap, &js, NULL) == NDT_OK;
            } else {
                /* rows from several contexts: gathered into host memory, encoded from there on the first context */
                unsigned char *rgba8 = (unsigned char *)malloc((size_t)width * height * 4);
                ok = rgba8 && ndt_hip_render_multi(g_ctx, g_n_ctx, &p, NDT_IMAGE_RGBA8, rgba8, NULL) == NDT_OK &&
                     ndt_hip_encode_jpeg(g_ctx[0], rgba8, width, height, &jo->jp, buf, cap, &js) == NDT_OK;
                free(rgba8);
            }
            if (ok) {
                say_jpeg(&js);
                *jo->jpg = buf;
                *jo->bytes = js.jpeg_bytes;
            } else free(buf);
        } else if (format == NDT_HOST_IMAGE_DEPTH8) {
            ok = render_depth8(&p, (depth_out *)out);
        } else if (depth)      /* the depth map comes from the one-context call (a map is not split over devices) */
            ok = format == NDT_IMAGE_F64 && ndt_hip_render_depth(g_ctx[0], &p, (double *)out, depth, NULL) == NDT_OK;
        else
            ok = ndt_hip_render_multi(g_ctx, g_n_ctx, &p, format, out, NULL) == NDT_OK;
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
        if (format == NDT_HOST_IMAGE_DEPTH8 && ok)
            fprintf(stderr, "ndt_render_image: bounds + kd-tree + flatten %.2f ms (%s), upload %.2f ms, render + 8-bit image and depth map to host %.2f ms (depth map finished on the GPU %.2f%s)\n",
                    NDT_MS(ts0, ts1), share, NDT_MS(ts1, ts2), NDT_MS(ts2, ts3), g_depth_ms,
                    ((depth_out *)out)->want_png ? ", image files made there" : "");
        else if (format == NDT_HOST_IMAGE_APNG && ok)
            fprintf(stderr, "ndt_render_image: bounds + kd-tree + flatten %.2f ms (%s), upload %.2f ms, render + the frame's bytes of the animated PNG to host %.2f ms (plan and file bytes on the GPU %.2f)\n",
                    NDT_MS(ts0, ts1), share, NDT_MS(ts1, ts2), NDT_MS(ts2, ts3), g_apng_ms);
        else if ((format == NDT_HOST_IMAGE_PNG || format == NDT_HOST_IMAGE_JPEG || format == NDT_HOST_IMAGE_PNG16 ||
                  format == NDT_HOST_IMAGE_PNG16_DEPTH) && ok)
            fprintf(stderr, "ndt_render_image: bounds + kd-tree + flatten %.2f ms (%s), upload %.2f ms, render + image file to host %.2f ms (image file on the GPU %.2f)\n",
                    NDT_MS(ts0, ts1), share, NDT_MS(ts1, ts2), NDT_MS(ts2, ts3), format == NDT_HOST_IMAGE_JPEG ? g_jpeg_ms : g_png_ms);
        else
            fprintf(stderr, "ndt_render_image: bounds + kd-tree + flatten %.2f ms (%s), upload %.2f ms, render + image to host %.2f ms\n",
                    NDT_MS(ts0, ts1), share, NDT_MS(ts1, ts2), NDT_MS(ts2, ts3));
        if (ssaa != 1 && ok)
            fprintf(stderr, "ndt_render_image: of the render, supersampling %dx%d: the folds on the GPU %.2f ms\n", ssaa, ssaa, g_ssaa_ms);
    }
    ndt_flat_builder_free(&fb);
    return ok;
}

/* everything render_image takes (ndt.c:900): samples = `-n`, stereo = the reference's stereo_mode (MONO ..
 * ANAGLYPH_3D), specular = specular_enabled (`-p` clears it), depth = the depth map of `-z` (width*height doubles) or NULL */
int ndt_render_image_full(scene *scn, int width, int height, int samples, int threads, int aa_diff, int aa_depth, int stereo,
                          int specular, int max_optic_depth, double *rgba, double *depth)
{
    /* (the pthread fan-out of ndt.c:949-975 is the GPU's job now; `threads` fits the scene's bounding spheres in parallel) */
    return render_any(scn, width, height, samples, aa_diff, aa_depth, stereo, specular, max_optic_depth, NDT_IMAGE_F64, rgba, depth, threads, 1);
}

int ndt_render_image_rgba8(scene *scn, int width, int height, int samples, int threads, int aa_diff, int aa_depth, int stereo,
                           int specular, int max_optic_depth, unsigned char *rgba8)
{
    return render_any(scn, width, height, samples, aa_diff, aa_depth, stereo, specular, max_optic_depth, NDT_IMAGE_RGBA8, rgba8, NULL, threads, 1);
}

int ndt_render_image_depth8(scene *scn, int width, int height, int samples, int threads, int aa_diff, int aa_depth, int stereo,
                            int specular, int max_optic_depth, int want_png, int want_depth_png, ndt_depth_frame *out)
{
    depth_out d = { out, want_png != 0, want_png && want_depth_png };
    memset(out, 0, sizeof(*out));
    g_depth_ms = 0.0;
    if (!render_any(scn, width, height, samples, aa_diff, aa_depth, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_DEPTH8, &d, NULL, threads, 1)) {
        ndt_depth_frame_free(out);
        return 0;
    }
    return 1;
}

int ndt_render_image_png(scene *scn, int width, int height, int samples, int threads, int aa_diff, int aa_depth, int stereo,
                         int specular, int max_optic_depth, unsigned char **png, long long *png_bytes)
{
    png_out po = { png, png_bytes };
    *png = NULL;
    *png_bytes = 0;
    return render_any(scn, width, height, samples, aa_diff, aa_depth, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_PNG, &po, NULL, threads, 1);
}

int ndt_render_image_jpeg(scene *scn, int width, int height, int samples, int threads, int aa_diff, int aa_depth, int stereo,
                          int specular, int max_optic_depth, int quality, int sampling, unsigned char **jpg, long long *jpg_bytes)
{
    jpeg_out jo = { jpg, jpg_bytes, jpeg_params_of(quality, sampling) };
    *jpg = NULL;
    *jpg_bytes = 0;
    return render_any(scn, width, height, samples, aa_diff, aa_depth, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_JPEG, &jo, NULL, threads, 1);
}

/* ---- the same calls for a frame supersampled ssaa x ssaa on the GPU (no -a beside it: the library refuses the pair) */
int ndt_render_image_ssaa_full(scene *scn, int width, int height, int samples, int threads, int stereo, int specular, int max_optic_depth,
                               int ssaa, double *rgba, double *depth)
{
    return render_any(scn, width, height, samples, -1, -1, stereo, specular, max_optic_depth, NDT_IMAGE_F64, rgba, depth, threads, ssaa);
}

int ndt_render_image_ssaa_rgba8(scene *scn, int width, int height, int samples, int threads, int stereo, int specular, int max_optic_depth,
                                int ssaa, unsigned char *rgba8)
{
    return render_any(scn, width, height, samples, -1, -1, stereo, specular, max_optic_depth, NDT_IMAGE_RGBA8, rgba8, NULL, threads, ssaa);
}

int ndt_render_image_ssaa_png(scene *scn, int width, int height, int samples, int threads, int stereo, int specular, int max_optic_depth,
                              int ssaa, unsigned char **png, long long *png_bytes)
{
    png_out po = { png, png_bytes };
    *png = NULL;
    *png_bytes = 0;
    return render_any(scn, width, height, samples, -1, -1, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_PNG, &po, NULL, threads, ssaa);
}

int ndt_render_image_ssaa_jpeg(scene *scn, int width, int height, int samples, int threads, int stereo, int specular, int max_optic_depth,
                               int ssaa, int quality, int sampling, unsigned char **jpg, long long *jpg_bytes)
{
    jpeg_out jo = { jpg, jpg_bytes, jpeg_params_of(quality, sampling) };
    *jpg = NULL;
    *jpg_bytes = 0;
    return render_any(scn, width, height, samples, -1, -1, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_JPEG, &jo, NULL, threads, ssaa);
}

int ndt_render_image_ssaa_depth8(scene *scn, int width, int height, int samples, int threads, int stereo, int specular, int max_optic_depth,
                                 int ssaa, int want_png, int want_depth_png, ndt_depth_frame *out)
{
    depth_out d = { out, want_png != 0, want_png && want_depth_png };
    memset(out, 0, sizeof(*out));
    g_depth_ms = 0.0;
    if (!render_any(scn, width, height, samples, -1, -1, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_DEPTH8, &d, NULL, threads, ssaa)) {
        ndt_depth_frame_free(out);
        return 0;
    }
    return 1;
}

/* ---- the frame's files at 16 bits a sample (`ndt_hip --png16`); ssaa = 1: the plain frame, with -a when aa_depth >= 0 */
int ndt_render_image_png16(scene *scn, int width, int height, int samples, int threads, int aa_diff, int aa_depth, int stereo,
                           int specular, int max_optic_depth, int ssaa, unsigned char **png, long long *png_bytes)
{
    png_out po = { png, png_bytes };
    *png = NULL;
    *png_bytes = 0;
    return render_any(scn, width, height, samples, aa_diff, aa_depth, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_PNG16, &po, NULL, threads, ssaa);
}

int ndt_render_image_png16_depth(scene *scn, int width, int height, int samples, int threads, int aa_diff, int aa_depth, int stereo,
                                 int specular, int max_optic_depth, int ssaa, ndt_depth_frame *out)
{
    memset(out, 0, sizeof(*out));
    g_depth_ms = 0.0;
    if (!render_any(scn, width, height, samples, aa_diff, aa_depth, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_PNG16_DEPTH, out, NULL, threads, ssaa)) {
        ndt_depth_frame_free(out);
        return 0;
    }
    return 1;
}

/* ---- the next frame of the animated PNG ndt_apng_begin opened (`ndt_hip --apng`); ssaa = 1: the plain frame, with -a when aa_depth >= 0 */
int ndt_render_image_apng_frame(scene *scn, int width, int height, int samples, int threads, int aa_diff, int aa_depth, int stereo,
                                int specular, int max_optic_depth, int ssaa, unsigned char **bytes, long long *n_bytes)
{
    png_out po = { bytes, n_bytes };
    *bytes = NULL;
    *n_bytes = 0;
    return render_any(scn, width, height, samples, aa_diff, aa_depth, stereo, specular, max_optic_depth, NDT_HOST_IMAGE_APNG, &po, NULL, threads, ssaa);
}
