/* ndt_main.c -- minimal frame-loop driver around the GPU path, accepting the flags the
 * BASELINE configs use (reference ndt.c:1450: -d -r -f -l -s -t -u -o).  It loads a scene
 * program exactly like the reference does (dlopen + dlsym scene_setup / scene_frames /
 * scene_cleanup, ndt.c:1654-1664), renders each frame with ndt_render_frame and writes
 * images/<scene>/<N>d/<WxH>/<scene>_<WxH>_<frame>.ppm (binary PPM of the pixel_d2c bytes), or with `--png` the 8-bit RGBA
 * PNG the reference writes by default (stored blocks from the host, or compressed by the GPU), or with `--jpeg` the baseline JPEG
 * its libjpeg build writes (made by the GPU: ndt_hip_render_jpeg; quality 95 and 4:2:0 like the reference's, or
 * `--jpeg-quality Q`, `--jpeg-sampling 420|444`).  `-z` adds the
 * normalised depth map, depth/<scene>_<WxH>_<frame>.ppm.  `--dump-scene F` writes the flattened
 * scene of the last frame as an ndtscene file instead of rendering.  `--fit gpu` fits the frames'
 * bounding spheres on the GPU (ndt_hip_fit_spheres) instead of on the host's `-t` threads; `--kd gpu` builds their kd-trees
 * there (ndt_hip_build_kdtree) instead of on the host; `--png --deflate gpu` has the GPU make the frame's PNG file, compressed
 * (ndt_hip_render_png), instead of the host's stored-block writer; `-z --depth gpu` has the GPU normalise and quantise the depth
 * map (ndt_hip_render_rgba8_depth) instead of sending it and the image back in doubles, and `--depth-png` then writes the map as a
 * PNG compressed there as well.  `--ssaa K` (1 .. 8, default 1) supersamples every frame K x K on the GPU: K renders of the frame
 * K times the size, folded there into a box-filtered average in linear light before anything is quantised (ndt_hip_render_ssaa*);
 * with every output flag, -m s|o|a, -n, -g and -j, not with -a or -m h.  `--png16` (with `--png --deflate gpu`) has the GPU make
 * the PNG at 16 bits a sample from the double framebuffer (ndt_hip_render_png16), and with `-z --depth gpu --depth-png` the map's
 * file as 16-bit grey; on one GPU context a frame (not with -g N > 1).  `--apng` writes all frames of `-f a:b` into ONE animated
 * PNG, images/<scene>/<N>d/<WxH>/<scene>_<WxH>.apng, instead of a file a frame: the GPU keeps the previous frame, finds the
 * rectangle that changed and compresses only that (ndt_hip_render_apng_frame); `--apng-fps F` (1 .. 1000, default 24) shows each
 * frame 1 / F seconds.  With --ssaa, -a, -n, -m and --fit / --kd gpu; it is the run's one colour file (not with --png, --jpeg,
 * --raw, --png16 or -z), and its frames meet one canvas in order (not with -g N > 1 or -j K > 1).  `--exr` writes every frame as an
 * OpenEXR file, ....exr where the PNG would be: the doubles as they are, in linear light (no clamp, no square root), as half samples
 * or with `--exr-pixel float` as floats, ZIP-compressed on the GPU (ndt_hip_render_exr); with `-z` the map is the file's Z channel,
 * unstretched, and no depth/ file is written.  With --ssaa, -a, -n, -m s|o|a and -j; it is the run's colour file (not with --png,
 * --jpeg, --raw, --png16 or --apng), the map needs no finish (not with --depth gpu or --depth-png), and one context makes it (not
 * with -g N > 1).  `--exr --exr-aov id,position,normal` (or `all`; any order, repeats allowed) adds what every pixel shows to that
 * file: the object its primary ray hits (channel id, UINT: object index + 1, 0 for none), the hit point in all N coordinates (P.00 ..,
 * FLOAT) and the normal there (N.00 .., FLOAT), found on the GPU by a feature pass beside the render (ndt_hip_render_exr_features).
 * With -z, --ssaa, -m s|o, -j, --fit gpu and --kd gpu; not with -a, -n above 1 or -m a|h, where a pixel has no single primary ray.
 * `--denoise [K]` (1 .. 6 iterations, default 4) denoises every frame on the GPU between the render and the sink: an edge-avoiding
 * a-trous wavelet over the doubles, in linear light, before anything is quantised, guided by the object, N-D hit point and N-D
 * normal of every pixel's primary ray (ndt_hip_render_denoised*); `--denoise-colour X`, `--denoise-plane X` (above 0, default 0.25
 * each) and `--denoise-normal E` (0 .. 8, default 5) set its three weights.  With the default stored PNG, --png [--deflate gpu],
 * --jpeg, --exr, --raw, -n, -j, --fit gpu and --kd gpu; not with -a, -m other than mono, -g N > 1, --ssaa above 1, --apng, --png16,
 * -z or --exr-aov.
 * `--sample-cap C` (1 .. 10000) makes -n an exact count where C <= n: no pixel takes more than C samples (without it a pixel samples
 * on while its mean moves by more than 1/256).  `--vdenoise [K]` (1 .. 6 iterations, default 4) is the same stage with the width
 * of the colour weight taken from the frame's own samples, pixel by pixel (ndt_hip_render_vdenoised*): it filters where the frame is
 * noisy and copies a pixel that has converged; `--vdenoise-colour X` (above 0, default 4: standard deviations), `--vdenoise-plane X`
 * and `--vdenoise-normal E` as above.  It goes with and without what --denoise does, and not with --denoise.
 * `--ao [K]` (1 .. 256 samples, default 16) shades every frame by its ambient occlusion, found on the GPU between the render and the
 * sink: from the N-D hit point of every pixel's primary ray K rays over the hemisphere of the N-D normal there, and the colour
 * multiplied by the cosine-weighted share of them that get away (ndt_hip_render_ao_shaded*); `--ao-radius R` (finite, 0 or above;
 * default 0: any hit occludes) lets only hits nearer than R occlude, `--ao-strength S` (0 .. 1, default 1) blends the factor towards
 * 1, `--ao-seed X` picks another set of sample streams.  With the default PPM, --png [--deflate gpu], --jpeg, --raw and --exr [-z]
 * [--exr-aov ...], whose file also gets the FLOAT channel AO (ndt_hip_render_exr_ao); with -n, -m s|o, -j, --fit gpu and --kd gpu; not
 * with -a, -m a|h, -g N > 1, --ssaa above 1, --apng, --png16, --denoise, --depth gpu or -z without --exr.
 * None falls back: what the device path cannot do ends the run. */
#include <dlfcn.h>
#include <errno.h>
#include <getopt.h>
#include <pthread.h>
#include <sys/stat.h>
#include <sys/time.h>

#include "ndt_host_internal.h"

static double now_s(void)
{
    struct timeval tv;
    gettimeofday(&tv, NULL);
    return tv.tv_sec + 1e-6 * tv.tv_usec;
}

static int write_png(const char *path, const unsigned char *rgba8, int w, int h);

/* both writers take the bytes the reference stores: pixel_d2c of every channel (image.h:36-39, image.c:648-651) */
static int write_ppm(const char *path, const unsigned char *rgba8, int w, int h)
{
    FILE *f = fopen(path, "wb");
    if (!f) return -1;
    fprintf(f, "P6\n%d %d\n255\n", w, h);
    unsigned char *row = (unsigned char *)malloc((size_t)w * 3);
    for (int j = 0; j < h; ++j) {
        for (int i = 0; i < w; ++i)
            for (int c = 0; c < 3; ++c) row[3 * i + c] = rgba8[((size_t)j * w + i) * 4 + c];
        fwrite(row, 1, (size_t)w * 3, f);
    }
    free(row);
    fclose(f);
    return 0;
}

/* a finished buffer as the file `path` (mode "wb"), or behind what the file holds ("ab"); a file that cannot be written ends the run */
static int write_bytes(const char *path, const char *mode, const void *bytes, size_t n)
{
    FILE *f = fopen(path, mode);
    int ok = f && fwrite(bytes, 1, n, f) == n;
    if (f && fclose(f) != 0) ok = 0;
    if (!ok) fprintf(stderr, "ndt_hip: cannot write %s\n", path);
    return ok;
}

/* pixel_d2c on the host: only for images that are in doubles here anyway (--raw, the normalised depth map) */
static unsigned char *quantise(const double *rgba, long n_values)
{
    unsigned char *out = (unsigned char *)malloc((size_t)n_values);
    for (long i = 0; i < n_values; ++i) {
        double d = rgba[i];
        double m = (1.0 < d) ? 1.0 : d;
        m = (0.0 > m) ? 0.0 : m;
        out[i] = (unsigned char)(sqrt(m) * 255);
    }
    return out;
}


/* ---- one frame: flatten, upload, render, save (what follows scene_setup in the reference's frame loop) */
/* what every frame asks of ndt_render_frame: main turns the flags into it, once */
static ndt_frame_request frame_request;
/* ... and what the run needs beside it */
static struct {
    int dims, gpus;
    int png;                        /* --png: 8-bit pixels that come back are written as a stored PNG, not a PPM */
    ndt_colour_kind host_file;      /* NDT_COLOUR_PNG / _JPEG: the frame comes back in doubles (--raw, a host-finished -z) and the file of
                                     * --png --deflate gpu / --jpeg is encoded on the GPU from the host's bytes; otherwise NDT_COLOUR_F64 */
    int apng_fps, apng_frames;      /* --apng: the animated PNG's frame rate; frames the run renders */
    const char *raw_path;
} job_opts;

/* images/<scene>/<N>d/<WxH>, made if need be */
static void image_dir(char *dir, size_t len, const scene *scn)
{
    mkdir("images", 0700);
    snprintf(dir, len, "images/%s", scn->name); mkdir(dir, 0700);
    snprintf(dir, len, "images/%s/%id", scn->name, job_opts.dims); mkdir(dir, 0700);
    snprintf(dir, len, "images/%s/%id/%ix%i", scn->name, job_opts.dims, frame_request.width, frame_request.height); mkdir(dir, 0700);
}

/* --apng: the run's one file, begun at the first frame, appended to per frame, closed by apng_close */
static char apng_path[1024];
static int apng_begun = 0;

static int render_frame_apng(scene *scn)
{
    const int width = frame_request.width, height = frame_request.height;
    ndt_frame f;
    const double t0 = now_s();
    if (!apng_begun && !ndt_apng_begin(width, height, job_opts.apng_frames, job_opts.apng_fps)) return 0;
    apng_begun = 1;
    /* the 8-bit image stays on the device: what comes back are the bytes to append */
    if (!ndt_render_frame(scn, &frame_request, &f)) return 0;
    printf("rendering took %.3fs\n", now_s() - t0);
    const double t_file = now_s();
    const int first = !apng_path[0];
    if (first) {
        char dir[512];
        image_dir(dir, sizeof(dir), scn);
        snprintf(apng_path, sizeof(apng_path), "%s/%s_%ix%i.apng", dir, scn->name, width, height);
    }
    const int ok = write_bytes(apng_path, first ? "wb" : "ab", f.file, (size_t)f.file_bytes);
    if (ok) printf("\tappended %lld bytes to %s\n", f.file_bytes, apng_path);
    if (ok && getenv("NDT_HOST_TIMING"))
        fprintf(stderr, "ndt_hip: image file %.2f ms (frame planned and compressed on the GPU %.2f, appended %.2f)\n",
                (now_s() - t_file) * 1e3 + f.file_ms, f.file_ms, (now_s() - t_file) * 1e3);
    ndt_frame_free(&f);
    return ok;
}

/* IEND behind the last frame */
static int apng_close(void)
{
    unsigned char tail[16];
    long long n = 0;
    if (!apng_path[0]) return 1;
    if (!ndt_apng_end(tail, &n) || !write_bytes(apng_path, "ab", tail, (size_t)n)) {
        fprintf(stderr, "ndt_hip: cannot finish %s\n", apng_path);
        return 0;
    }
    printf("\tsaved %s\n", apng_path);
    return 1;
}

/* the colour file of frame i from what arrived: a file made on the GPU as it is; pixels as a PPM or a stored PNG, or (host_file)
 * as the file the GPU makes of them */
static int save_colour(const scene *scn, int i, ndt_frame *f)
{
    const int width = frame_request.width, height = frame_request.height;
    const int on_host = f->file == NULL;       /* the image is in host memory */
    const ndt_colour_kind kind = on_host ? job_opts.host_file : frame_request.colour;
    const double t_file = now_s();
    char dir[512], path[1024];
    if (kind == NDT_COLOUR_JPEG && on_host &&
        !ndt_encode_image_jpeg(f->rgba8, width, height, frame_request.jpeg_quality, frame_request.jpeg_sampling, &f->file, &f->file_bytes, &f->file_ms)) return 0;
    if (kind == NDT_COLOUR_PNG && on_host && !ndt_encode_image_png(f->rgba8, width, height, &f->file, &f->file_bytes, &f->file_ms)) return 0;
    image_dir(dir, sizeof(dir), scn);
    snprintf(path, sizeof(path), "%s/%s_%ix%i_%04i.%s", dir, scn->name, width, height, i,
             kind == NDT_COLOUR_EXR ? "exr" : kind == NDT_COLOUR_JPEG ? "jpg" : job_opts.png ? "png" : "ppm");
    if (f->file) {
        if (!write_bytes(path, "wb", f->file, (size_t)f->file_bytes)) return 0;
    } else if (job_opts.png) write_png(path, f->rgba8, width, height);
    else write_ppm(path, f->rgba8, width, height);
    printf("\tsaved %s\n", path);
    if (getenv("NDT_HOST_TIMING")) {
        /* a file made where the image is: the encoder's share is inside "rendering took" */
        const double ms = (now_s() - t_file) * 1e3;
        if (f->file) fprintf(stderr, "ndt_hip: image file %.2f ms (%s on the GPU %.2f, written %.2f)\n", on_host ? ms : ms + f->file_ms,
                             kind == NDT_COLOUR_JPEG ? "JPEG made" : kind == NDT_COLOUR_EXR ? "EXR made" : "compressed", f->file_ms, on_host ? ms - f->file_ms : ms);
        else fprintf(stderr, "ndt_hip: image file %.2f ms (%s, made and written by the host)\n", ms, job_opts.png ? "stored PNG" : "PPM");
    }
    return 1;
}

/* the map file of -z: depth/<scene>_<WxH>_<frame>.ppm, or .png */
static int save_map(const scene *scn, int i, const ndt_frame *f)
{
    const int width = frame_request.width, height = frame_request.height;
    const double t_depth = now_s();
    char path[1024];
    mkdir("depth", 0700);
    snprintf(path, sizeof(path), "depth/%s_%ix%i_%04i.%s", scn->name, width, height, i, f->depth_file ? "png" : "ppm");
    if (f->depth) {
        /* dbl_image_normalize (image.c:1025-1065) stretches the map to 0..1 before it is saved (ndt.c:1010-1016) */
        double lo = f->depth[0], hi = f->depth[0];
        for (long k = 0; k < (long)width * height; ++k) {
            if (f->depth[k] < lo) lo = f->depth[k];
            if (f->depth[k] > hi) hi = f->depth[k];
        }
        double *norm = (double *)malloc((size_t)width * height * 4 * sizeof(double));
        for (long k = 0; k < (long)width * height; ++k) {
            const double v = hi > lo ? (f->depth[k] - lo) / (hi - lo) : 0.0;
            norm[4 * k] = norm[4 * k + 1] = norm[4 * k + 2] = v;
            norm[4 * k + 3] = 1.0;
        }
        unsigned char *norm8 = quantise(norm, (long)width * height * 4);
        write_ppm(path, norm8, width, height);
        printf("\tsaved %s\n", path);
        free(norm8);
        free(norm);
        return 1;
    }
    /* the map arrived normalised and quantised (or as its file): only the writing is left */
    if (!f->depth_file) write_ppm(path, f->depth8, width, height);
    else if (!write_bytes(path, "wb", f->depth_file, (size_t)f->depth_file_bytes)) return 0;
    printf("\tsaved %s\n", path);
    if (getenv("NDT_HOST_TIMING"))
        fprintf(stderr, "ndt_hip: depth file %.2f ms (map finished on the GPU %.2f, inside \"rendering took\"; %s written by the host)\n",
                (now_s() - t_depth) * 1e3, f->depth_ms, f->depth_file ? "PNG made there," : "PPM made and");
    return 1;
}

/* --raw F: the doubles as they arrived, the map's in F.depth */
static int save_raw(const ndt_frame *f)
{
    const size_t n = (size_t)frame_request.width * frame_request.height;
    char dpath[1100];
    snprintf(dpath, sizeof(dpath), "%s.depth", job_opts.raw_path);
    return (!f->depth || write_bytes(dpath, "wb", f->depth, n * sizeof(double))) &&
           write_bytes(job_opts.raw_path, "wb", f->rgba, n * 4 * sizeof(double));
}

static int render_frame(scene *scn, int i)
{
    if (frame_request.colour == NDT_COLOUR_APNG) return render_frame_apng(scn);
    ndt_frame f;
    const double t0 = now_s();
    if (!ndt_render_frame(scn, &frame_request, &f)) return 0;
    /* doubles came back: the host makes the bytes of the colour file */
    if (f.rgba) f.rgba8 = quantise(f.rgba, (long)frame_request.width * frame_request.height * 4);
    printf("rendering took %.3fs\n", now_s() - t0);
    const int ok = save_colour(scn, i, &f) && (frame_request.map == NDT_MAP_NONE || frame_request.map == NDT_MAP_EXR_Z || save_map(scn, i, &f)) &&
                   (!job_opts.raw_path || save_raw(&f));
    ndt_frame_free(&f);
    return ok;
}

/* ---- bounded queue of frames between the scene program (producer) and the render workers */
typedef struct { scene *scn; int frame; } frame_job;
static frame_job *queue = NULL;
static int queue_cap = 0, queue_n = 0, queue_head = 0, queue_done = 0, worker_failed = 0;
static pthread_mutex_t queue_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t queue_not_full = PTHREAD_COND_INITIALIZER, queue_not_empty = PTHREAD_COND_INITIALIZER;

static void queue_push(scene *scn, int frame)
{
    pthread_mutex_lock(&queue_mu);
    while (queue_n == queue_cap) pthread_cond_wait(&queue_not_full, &queue_mu);
    queue[(queue_head + queue_n) % queue_cap].scn = scn;
    queue[(queue_head + queue_n) % queue_cap].frame = frame;
    ++queue_n;
    pthread_cond_signal(&queue_not_empty);
    pthread_mutex_unlock(&queue_mu);
}

static void queue_close(void)
{
    pthread_mutex_lock(&queue_mu);
    queue_done = 1;
    pthread_cond_broadcast(&queue_not_empty);
    pthread_mutex_unlock(&queue_mu);
}

static void *worker_main(void *arg)
{
    /* worker w renders its frames on device w mod device count: one frame per GPU, the reference's MPI_MODE_FRAME
     * (ndt.c:1770-1830); with -g n every frame is spread over n contexts instead */
    const int w = (int)(long)arg;
    const int n_dev = ndt_hip_device_count();
    if (job_opts.gpus > 1) ndt_render_use_devices(job_opts.gpus);
    else ndt_render_use_device(n_dev > 0 ? w % n_dev : 0);
    for (;;) {
        pthread_mutex_lock(&queue_mu);
        while (queue_n == 0 && !queue_done) pthread_cond_wait(&queue_not_empty, &queue_mu);
        if (queue_n == 0) {
            pthread_mutex_unlock(&queue_mu);
            return NULL;
        }
        frame_job j = queue[queue_head];
        queue_head = (queue_head + 1) % queue_cap;
        --queue_n;
        pthread_cond_signal(&queue_not_full);
        pthread_mutex_unlock(&queue_mu);
        if (!render_frame(j.scn, j.frame)) worker_failed = 1;
        scene_free(j.scn);
        free(j.scn);
    }
}

/* scenes/yaml.c:14-50 */
static int yaml_scene_frames(int dimensions, char *config)
{
    if (config == NULL || dimensions < 3) return 0;
    return scene_yaml_count_frames(config);
}

static int yaml_scene_setup(scene *scn, int dimensions, int frame, int frames, char *config)
{
    (void)frames;
    scene_init(scn, "nameless", dimensions);
    if (config == NULL) {
        fprintf(stderr, "YAML scene requires a filename, use `-u filename`.\n");
        exit(1);
    }
    scene_read_yaml(scn, config, frame);
    return 0;
}

/* ---- PNG, 8-bit RGBA like the reference's writer (image.c:563-660: PNG_COLOR_TYPE_RGB_ALPHA, pixel_d2c on every
 * channel), without libpng: the zlib stream inside IDAT uses stored (uncompressed) deflate blocks */
static unsigned int crc_table[256];
static void crc_init(void)
{
    for (unsigned int n = 0; n < 256; ++n) {
        unsigned int c = n;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        crc_table[n] = c;
    }
}
static unsigned int crc_update(unsigned int c, const unsigned char *buf, size_t len)
{
    for (size_t i = 0; i < len; ++i) c = crc_table[(c ^ buf[i]) & 0xff] ^ (c >> 8);
    return c;
}
static void put_be32(unsigned char *p, unsigned int v) { p[0] = v >> 24; p[1] = v >> 16; p[2] = v >> 8; p[3] = v; }
static void png_chunk(FILE *f, const char *type, const unsigned char *data, size_t len)
{
    unsigned char hdr[8];
    put_be32(hdr, (unsigned int)len);
    memcpy(hdr + 4, type, 4);
    fwrite(hdr, 1, 8, f);
    if (len) fwrite(data, 1, len, f);
    unsigned int c = crc_update(0xffffffffu, hdr + 4, 4);
    c = crc_update(c, data, len) ^ 0xffffffffu;
    unsigned char tail[4];
    put_be32(tail, c);
    fwrite(tail, 1, 4, f);
}

static int write_png(const char *path, const unsigned char *rgba8, int w, int h)
{
    FILE *f = fopen(path, "wb");
    if (!f) return -1;
    crc_init();
    static const unsigned char sig[8] = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
    fwrite(sig, 1, 8, f);
    unsigned char ihdr[13];
    put_be32(ihdr, (unsigned int)w);
    put_be32(ihdr + 4, (unsigned int)h);
    ihdr[8] = 8; ihdr[9] = 6; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;     /* 8 bit, RGBA, no interlace */
    png_chunk(f, "IHDR", ihdr, 13);
    /* raw image: one filter byte (0 = none) + 4 bytes per pixel, per row */
    const size_t row = 1 + (size_t)w * 4, raw_len = row * (size_t)h;
    unsigned char *raw = (unsigned char *)malloc(raw_len);
    for (int j = 0; j < h; ++j) {
        unsigned char *q = raw + (size_t)j * row;
        *q++ = 0;
        memcpy(q, rgba8 + (size_t)j * w * 4, (size_t)w * 4);
    }
    /* zlib: header, stored blocks of at most 65535 bytes, adler32 */
    const size_t n_blocks = (raw_len + 65534) / 65535;
    const size_t z_len = 2 + raw_len + 5 * (n_blocks ? n_blocks : 1) + 4;
    unsigned char *z = (unsigned char *)malloc(z_len), *zp = z;
    *zp++ = 0x78; *zp++ = 0x01;
    unsigned int a = 1, b = 0;
    size_t off = 0;
    do {
        size_t n = raw_len - off > 65535 ? 65535 : raw_len - off;
        *zp++ = (off + n == raw_len) ? 1 : 0;
        *zp++ = n & 0xff; *zp++ = (n >> 8) & 0xff; *zp++ = ~n & 0xff; *zp++ = (~n >> 8) & 0xff;
        memcpy(zp, raw + off, n);
        for (size_t i = 0; i < n; ++i) {        /* adler32; the modulo can wait 5552 bytes, but this is not the hot path */
            a = (a + raw[off + i]) % 65521u;
            b = (b + a) % 65521u;
        }
        zp += n;
        off += n;
    } while (off < raw_len);
    put_be32(zp, (b << 16) | a);
    zp += 4;
    png_chunk(f, "IDAT", z, (size_t)(zp - z));
    png_chunk(f, "IEND", NULL, 0);
    free(z);
    free(raw);
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    int dims = 3, width = 1920, height = 1080, first = 0, last = -1, frames = 300, frames_given = 0;
    int depth = 128, threads = 1;
    int aa_diff = 20, aa_depth = -1;        /* -a: recursive anti-aliasing off unless given (ndt.c:1411-1412, 1453) */
    int jobs = 1;           /* -j: frames in flight, worker w on GPU w mod device count (MPI_MODE_FRAME, ndt.c:1770-1830) */
    int gpus = 1;           /* -g: contexts ONE frame is spread over, context k on GPU k mod device count (MPI_MODE_ROW, ndt.c:812-820) */
    int png = 0;            /* --png: 8-bit RGBA PNG like the reference's default IMAGE_FORMAT (image.h:56-64) instead of PPM */
    int samples = 1;        /* -n (ndt.c:1574-1577) */
    int stereo = 0, specular = 1, want_depth = 0;      /* -m, -p, -z (ndt.c:1533-1573, 1581-1589, 1726-1729) */
    char *scene_path = NULL, *config = NULL, *dump_path = NULL, *raw_path = NULL;
    int fit_gpu = 0;        /* --fit host|gpu: where the frames' bounding spheres are fitted (default: host, on the -t threads) */
    int kd_gpu = 0;         /* --kd host|gpu: where the frames' kd-trees are built (default: host) */
    int depth_gpu = 0;      /* --depth host|gpu: who normalises and quantises the depth map of -z: the host, from doubles (default), or the GPU */
    int depth_png = 0;      /* --depth-png: the map as a PNG compressed on the GPU instead of a PPM (needs --depth gpu --png --deflate gpu) */
    int deflate_gpu = 0;    /* --deflate stored|gpu: who makes the --png file: the host, in stored blocks (default), or the GPU, compressed */
    int jpeg = 0;           /* --jpeg: the frame's file is the baseline JPEG the reference's libjpeg build writes (image.c:346-412), made on the GPU */
    int jpeg_quality = 0;   /* --jpeg-quality 1 .. 100 (default: the reference's 95) */
    int jpeg_sampling = -1; /* --jpeg-sampling 420|444 (default: 4:2:0, libjpeg's) */
    int ssaa = 1;           /* --ssaa K: every frame supersampled K x K on the GPU, 1 .. 8 (default 1: the plain frame) */
    int png16 = 0;          /* --png16: the PNG files at 16 bits a sample, made on the GPU from the doubles (needs --png --deflate gpu) */
    int apng = 0;           /* --apng: all frames of the run in one animated PNG, the difference between frames found on the GPU */
    int apng_fps = 0;       /* --apng-fps 1 .. 1000 (default 24): each frame is shown 1 / F seconds */
    int exr = 0;            /* --exr: the frame's file is an OpenEXR file of the doubles in linear light, made on the GPU; with -z the map is its Z channel */
    int exr_pixel = 0;      /* --exr-pixel half|float: the colour channels' samples, 1 / 2 (default: half) */
    int exr_aov = 0;        /* --exr-aov id,position,normal|all: what every pixel's primary ray hits, as channels id, P.*, N.* of the OpenEXR file (a mask of NDT_FEATURE_*) */
    int exr_aov_given = 0;
    int denoise = 0;        /* --denoise [K]: every frame denoised on the GPU by K iterations of the a-trous filter, 1 .. 6 (default 4); 0: off */
    int denoise_normal = 5; /* --denoise-normal E: the normals' dot product squared E times, 0 .. 8 */
    double denoise_colour = 0.25, denoise_plane = 0.25;     /* --denoise-colour X, --denoise-plane X: sigma_colour, sigma_plane, above 0 */
    const char *denoise_tuned = NULL;       /* the first --denoise-* flag given */
    int vdenoise = 0;       /* --vdenoise [K]: every frame denoised on the GPU by K iterations of the variance-guided a-trous filter, 1 .. 6 (default 4); 0: off */
    int vdenoise_normal = 5;    /* --vdenoise-normal E, 0 .. 8 */
    double vdenoise_colour = 4.0, vdenoise_plane = 0.25;    /* --vdenoise-colour X, --vdenoise-plane X: k_colour, sigma_plane, above 0 */
    const char *vdenoise_tuned = NULL;      /* the first --vdenoise-* flag given */
    int sample_cap = 0;     /* --sample-cap C: no pixel takes more than C samples (option "sample_cap"); 0: no cap, -n is a lower bound */
    int ao = 0;             /* --ao [K]: every frame shaded by its ambient occlusion of K samples a pixel, found on the GPU, 1 .. 256 (default 16); 0: off */
    double ao_radius = 0.0, ao_strength = 1.0;      /* --ao-radius R: finite, 0 (any hit occludes) or above; --ao-strength S: 0 .. 1 */
    unsigned long long ao_seed = 0;                 /* --ao-seed X */
    const char *ao_tuned = NULL;            /* the first --ao-* flag given */
    char *objects_dir = "objects";      /* -o: where object plugins are looked for (object.c:119; ndt.c passes "objects") */
    static struct option longopts[] = { { "dump-scene", required_argument, NULL, 1000 },
                                        { "raw", required_argument, NULL, 1001 }, { "png", no_argument, NULL, 1002 },
                                        { "fit", required_argument, NULL, 1003 }, { "kd", required_argument, NULL, 1004 },
                                        { "deflate", required_argument, NULL, 1005 },
                                        { "depth", required_argument, NULL, 1006 }, { "depth-png", no_argument, NULL, 1007 },
                                        { "jpeg", no_argument, NULL, 1008 }, { "jpeg-quality", required_argument, NULL, 1009 },
                                        { "jpeg-sampling", required_argument, NULL, 1010 }, { "ssaa", required_argument, NULL, 1011 },
                                        { "png16", no_argument, NULL, 1012 }, { "apng", no_argument, NULL, 1013 },
                                        { "apng-fps", required_argument, NULL, 1014 }, { "exr", no_argument, NULL, 1015 },
                                        { "exr-pixel", required_argument, NULL, 1016 }, { "exr-aov", required_argument, NULL, 1017 },
                                        { "denoise", optional_argument, NULL, 1018 }, { "denoise-colour", required_argument, NULL, 1019 },
                                        { "denoise-plane", required_argument, NULL, 1020 }, { "denoise-normal", required_argument, NULL, 1021 },
                                        { "ao", optional_argument, NULL, 1022 }, { "ao-radius", required_argument, NULL, 1023 },
                                        { "ao-strength", required_argument, NULL, 1024 }, { "ao-seed", required_argument, NULL, 1025 },
                                        { "vdenoise", optional_argument, NULL, 1026 }, { "vdenoise-colour", required_argument, NULL, 1027 },
                                        { "vdenoise-plane", required_argument, NULL, 1028 }, { "vdenoise-normal", required_argument, NULL, 1029 },
                                        { "sample-cap", required_argument, NULL, 1030 },
                                        { NULL, 0, NULL, 0 } };
    int ch;
    while ((ch = getopt_long(argc, argv, "a:d:g:r:f:j:l:m:3:n:ps:t:u:o:zh", longopts, NULL)) != -1) {
        int a1, a2, a3, n;
        switch (ch) {
        case 'a':       /* -a diff,depth (ndt.c:1453-1465); defaults 20,4 */
            aa_depth = 4;
            n = sscanf(optarg, "%d,%d", &a1, &a2);
            if (n >= 1) aa_diff = a1;
            if (n >= 2) aa_depth = a2;
            printf("anti-aliasing = diff=%i,depth=%i\n", aa_diff, aa_depth);
            break;
        case 'd': dims = atoi(optarg); break;
        case 'r':
            if (!strcmp(optarg, "4k")) { width = 3840; height = 2160; }
            else if (!strcmp(optarg, "1080p")) { width = 1920; height = 1080; }
            else if (!strcmp(optarg, "720p")) { width = 1280; height = 720; }
            else if (!strcmp(optarg, "480p")) { width = 720; height = 480; }
            else sscanf(optarg, "%dx%d", &width, &height);
            break;
        case 'f':       /* first:last:total, first:last, or last (ndt.c:1510-1524) */
            n = sscanf(optarg, "%d:%d:%d", &a1, &a2, &a3);
            if (n >= 3) { first = a1; last = a2; frames = a3; frames_given = 1; }
            else if (n >= 2) { first = a1; last = a2; }
            else if (n >= 1) { last = a1; }
            break;
        case 'g': gpus = atoi(optarg); break;
        case 'j': jobs = atoi(optarg); break;
        case 'l': depth = atoi(optarg); break;
        case 'm':
        case '3':       /* s(ide by side) / o(ver-under) / a(naglyph) / m(ono), ndt.c:1538-1572 */
            switch (optarg[0]) {
            case 'S': case 's': stereo = 1; printf("stereo = SIDE_SIDE_3D\n"); break;
            case 'O': case 'o': stereo = 2; printf("stereo = OVER_UNDER_3D\n"); break;
            case 'A': case 'a': stereo = 3; printf("stereo = ANAGLYPH_3D\n"); break;
            case 'H': case 'h': stereo = 4; width = 1920; height = 2205; printf("stereo = HIDEF_3D\n"); break;     /* ndt.c:1557-1565 */
            default: stereo = 0; printf("stereo = MONO\n"); break;
            }
            break;
        case 'n': samples = atoi(optarg); printf("samples = %i\n", samples); break;
        case 'p': specular = 0; printf("disabling specular highlights.\n"); break;
        case 'z': want_depth = 1; printf("record_depth_map = yes\n"); break;
        case 's': scene_path = optarg; break;
        case 't': threads = atoi(optarg); break;
        case 'u': config = optarg; break;
        case 'o': objects_dir = optarg; break;    /* object.c:119: a directory of object plugins (the built-in types need none) */
        case 1000: dump_path = optarg; break;
        case 1001: raw_path = optarg; break;
        case 1002: png = 1; break;
        case 1003:
            if (!strcmp(optarg, "gpu")) fit_gpu = 1;
            else if (!strcmp(optarg, "host")) fit_gpu = 0;
            else { fprintf(stderr, "%s: --fit takes host or gpu, not '%s'\n", argv[0], optarg); return 1; }
            break;
        case 1004:
            if (!strcmp(optarg, "gpu")) kd_gpu = 1;
            else if (!strcmp(optarg, "host")) kd_gpu = 0;
            else { fprintf(stderr, "%s: --kd takes host or gpu, not '%s'\n", argv[0], optarg); return 1; }
            break;
        case 1005:
            if (!strcmp(optarg, "gpu")) deflate_gpu = 1;
            else if (!strcmp(optarg, "stored")) deflate_gpu = 0;
            else { fprintf(stderr, "%s: --deflate takes stored or gpu, not '%s'\n", argv[0], optarg); return 1; }
            break;
        case 1006:
            if (!strcmp(optarg, "gpu")) depth_gpu = 1;
            else if (!strcmp(optarg, "host")) depth_gpu = 0;
            else { fprintf(stderr, "%s: --depth takes host or gpu, not '%s'\n", argv[0], optarg); return 1; }
            break;
        case 1007: depth_png = 1; break;
        case 1008: jpeg = 1; break;
        case 1009: {
            char *end = NULL;
            const long q = strtol(optarg, &end, 10);
            if (end == optarg || *end || q < 1 || q > 100) {
                fprintf(stderr, "%s: --jpeg-quality takes 1 .. 100, not '%s'\n", argv[0], optarg);
                return 1;
            }
            jpeg_quality = (int)q;
            break;
        }
        case 1010:
            if (!strcmp(optarg, "420")) jpeg_sampling = 0;
            else if (!strcmp(optarg, "444")) jpeg_sampling = 1;
            else { fprintf(stderr, "%s: --jpeg-sampling takes 420 or 444, not '%s'\n", argv[0], optarg); return 1; }
            break;
        case 1011: {
            char *end = NULL;
            const long k = strtol(optarg, &end, 10);
            if (end == optarg || *end || k < 1 || k > 8) {
                fprintf(stderr, "%s: --ssaa takes 1 .. 8, not '%s'\n", argv[0], optarg);
                return 1;
            }
            ssaa = (int)k;
            break;
        }
        case 1012: png16 = 1; break;
        case 1013: apng = 1; break;
        case 1014: {
            char *end = NULL;
            const long f = strtol(optarg, &end, 10);
            if (end == optarg || *end || f < 1 || f > 1000) {
                fprintf(stderr, "%s: --apng-fps takes 1 .. 1000, not '%s'\n", argv[0], optarg);
                return 1;
            }
            apng_fps = (int)f;
            break;
        }
        case 1015: exr = 1; break;
        case 1016:
            if (!strcmp(optarg, "half")) exr_pixel = 1;
            else if (!strcmp(optarg, "float")) exr_pixel = 2;
            else { fprintf(stderr, "%s: --exr-pixel takes half or float, not '%s'\n", argv[0], optarg); return 1; }
            break;
        case 1017: {
            /* words separated by commas, in any order, repeats allowed */
            const char *w = optarg;
            exr_aov_given = 1;
            for (;;) {
                const size_t len = strcspn(w, ",");
                if (len == 2 && !strncmp(w, "id", 2)) exr_aov |= NDT_FEATURE_ID;
                else if (len == 8 && !strncmp(w, "position", 8)) exr_aov |= NDT_FEATURE_POSITION;
                else if (len == 6 && !strncmp(w, "normal", 6)) exr_aov |= NDT_FEATURE_NORMAL;
                else if (len == 3 && !strncmp(w, "all", 3)) exr_aov |= NDT_FEATURE_ID | NDT_FEATURE_POSITION | NDT_FEATURE_NORMAL;
                else {
                    if (len == 0) fprintf(stderr, "%s: --exr-aov takes a list of id, position, normal (or all): an empty word in '%s'\n", argv[0], optarg);
                    else fprintf(stderr, "%s: --exr-aov takes a list of id, position, normal (or all), not '%.*s'\n", argv[0], (int)len, w);
                    return 1;
                }
                if (!w[len]) break;
                w += len + 1;
            }
            break;
        }
        case 1018: {
            /* --denoise, --denoise=K or --denoise K: a following word that starts with a digit is the count */
            const char *arg = optarg;
            if (!arg && optind < argc && argv[optind][0] >= '0' && argv[optind][0] <= '9') arg = argv[optind++];
            denoise = 4;
            if (arg) {
                char *end = NULL;
                const long k = strtol(arg, &end, 10);
                if (end == arg || *end || k < 1 || k > 6) {
                    fprintf(stderr, "%s: --denoise takes 1 .. 6 iterations, not '%s'\n", argv[0], arg);
                    return 1;
                }
                denoise = (int)k;
            }
            break;
        }
        case 1019:
        case 1020: {
            char *end = NULL;
            const double x = strtod(optarg, &end);
            const char *flag = ch == 1019 ? "--denoise-colour" : "--denoise-plane";
            if (end == optarg || *end || !(x > 0) || !isfinite(x)) {
                fprintf(stderr, "%s: %s takes a finite number above 0, not '%s'\n", argv[0], flag, optarg);
                return 1;
            }
            if (ch == 1019) denoise_colour = x;
            else denoise_plane = x;
            if (!denoise_tuned) denoise_tuned = flag;
            break;
        }
        case 1021: {
            char *end = NULL;
            const long e = strtol(optarg, &end, 10);
            if (end == optarg || *end || e < 0 || e > 8) {
                fprintf(stderr, "%s: --denoise-normal takes 0 .. 8, not '%s'\n", argv[0], optarg);
                return 1;
            }
            denoise_normal = (int)e;
            if (!denoise_tuned) denoise_tuned = "--denoise-normal";
            break;
        }
        case 1022: {
            /* --ao, --ao=K or --ao K: a following word that starts with a digit is the count */
            const char *arg = optarg;
            if (!arg && optind < argc && argv[optind][0] >= '0' && argv[optind][0] <= '9') arg = argv[optind++];
            ao = 16;
            if (arg) {
                char *end = NULL;
                const long k = strtol(arg, &end, 10);
                if (end == arg || *end || k < 1 || k > 256) {
                    fprintf(stderr, "%s: --ao takes 1 .. 256 samples, not '%s'\n", argv[0], arg);
                    return 1;
                }
                ao = (int)k;
            }
            break;
        }
        case 1023:
        case 1024: {
            char *end = NULL;
            const double x = strtod(optarg, &end);
            if (end == optarg || *end || !(x >= 0) || !isfinite(x) || (ch == 1024 && x > 1)) {
                if (ch == 1023) fprintf(stderr, "%s: --ao-radius takes a finite number, 0 or above, not '%s'\n", argv[0], optarg);
                else fprintf(stderr, "%s: --ao-strength takes 0 .. 1, not '%s'\n", argv[0], optarg);
                return 1;
            }
            if (ch == 1023) ao_radius = x;
            else ao_strength = x;
            if (!ao_tuned) ao_tuned = ch == 1023 ? "--ao-radius" : "--ao-strength";
            break;
        }
        case 1025: {
            char *end = NULL;
            errno = 0;
            ao_seed = strtoull(optarg, &end, 0);
            if (end == optarg || *end || errno || optarg[0] == '-') {
                fprintf(stderr, "%s: --ao-seed takes an unsigned 64-bit number, not '%s'\n", argv[0], optarg);
                return 1;
            }
            if (!ao_tuned) ao_tuned = "--ao-seed";
            break;
        }
        case 1026: {
            /* --vdenoise, --vdenoise=K or --vdenoise K: a following word that starts with a digit is the count */
            const char *arg = optarg;
            if (!arg && optind < argc && argv[optind][0] >= '0' && argv[optind][0] <= '9') arg = argv[optind++];
            vdenoise = 4;
            if (arg) {
                char *end = NULL;
                const long k = strtol(arg, &end, 10);
                if (end == arg || *end || k < 1 || k > 6) {
                    fprintf(stderr, "%s: --vdenoise takes 1 .. 6 iterations, not '%s'\n", argv[0], arg);
                    return 1;
                }
                vdenoise = (int)k;
            }
            break;
        }
        case 1027:
        case 1028: {
            char *end = NULL;
            const double x = strtod(optarg, &end);
            const char *flag = ch == 1027 ? "--vdenoise-colour" : "--vdenoise-plane";
            if (end == optarg || *end || !(x > 0) || !isfinite(x)) {
                fprintf(stderr, "%s: %s takes a finite number above 0, not '%s'\n", argv[0], flag, optarg);
                return 1;
            }
            if (ch == 1027) vdenoise_colour = x;
            else vdenoise_plane = x;
            if (!vdenoise_tuned) vdenoise_tuned = flag;
            break;
        }
        case 1029: {
            char *end = NULL;
            const long e = strtol(optarg, &end, 10);
            if (end == optarg || *end || e < 0 || e > 8) {
                fprintf(stderr, "%s: --vdenoise-normal takes 0 .. 8, not '%s'\n", argv[0], optarg);
                return 1;
            }
            vdenoise_normal = (int)e;
            if (!vdenoise_tuned) vdenoise_tuned = "--vdenoise-normal";
            break;
        }
        case 1030: {
            char *end = NULL;
            const long c = strtol(optarg, &end, 10);
            if (end == optarg || *end || c < 1 || c > 10000) {
                fprintf(stderr, "%s: --sample-cap takes 1 .. 10000 samples a pixel, not '%s'\n", argv[0], optarg);
                return 1;
            }
            sample_cap = (int)c;
            break;
        }
        default:
            fprintf(stderr, "usage: %s -s scene.so|builtin:yaml [-d dims] [-r WxH|1080p|4k] [-f last|first:last[:total]] [-l depth]\n"
                            "          [-a diff,depth] [-n samples] [-m s|o|a|m] [-p] [-z] [-j frames_in_flight] [-g gpus_per_frame] [-u config] [--dump-scene file.ndtscene] [--raw file.f64] [--png [--deflate stored|gpu]] [--jpeg [--jpeg-quality 1..100] [--jpeg-sampling 420|444]] [--fit host|gpu] [--kd host|gpu] [--depth host|gpu [--depth-png]] [--ssaa 1..8] [--png16] [--apng [--apng-fps 1..1000]] [--exr [--exr-pixel half|float] [--exr-aov id,position,normal|all]]\n"
                            "          [--denoise [1..6] [--denoise-colour X] [--denoise-plane X] [--denoise-normal 0..8]]: every frame denoised on the GPU, with the stored PNG, --png [--deflate gpu], --jpeg, --exr, --raw, -n, -j, --fit gpu, --kd gpu; refused with -a, -m s|o|a|h, -g N > 1, --ssaa above 1, --apng, --png16, -z, --exr-aov\n"
                            "          [--sample-cap C]: no pixel takes more than C samples (without it -n is a lower bound: a pixel samples on while its mean moves by more than 1/256)\n"
                            "          [--vdenoise [1..6] [--vdenoise-colour X] [--vdenoise-plane X] [--vdenoise-normal 0..8]]: every frame denoised on the GPU by the variance-guided filter, which takes the width of its colour weight from the frame's own samples (best with -n K --sample-cap K); goes with and is refused with what --denoise is, and with --denoise\n"
                            "          [--ao [1..256] [--ao-radius R] [--ao-strength 0..1] [--ao-seed X]]: every frame shaded by its ambient occlusion, found on the GPU, with the PPM, --png [--deflate gpu], --jpeg, --raw, --exr [-z] [--exr-aov ...] (which gets the channel AO), -n, -m s|o, -j, --fit gpu, --kd gpu; refused with -a, -m a|h, -g N > 1, --ssaa above 1, --apng, --png16, --denoise, --depth gpu, -z without --exr\n", argv[0]);
            return ch == 'h' ? 0 : 1;
        }
    }
    if (!scene_path || dims < 3 || width < 1 || height < 1) {
        fprintf(stderr, "%s: need -s scene.so, dims >= 3 and a resolution\n", argv[0]);
        return 1;
    }
    if (ao_tuned && !ao) {
        fprintf(stderr, "%s: %s sets a parameter of the ambient occlusion: it needs --ao\n", argv[0], ao_tuned);
        return 1;
    }
    if (ao && aa_depth >= 0) {
        fprintf(stderr, "%s: --ao with -a: an anti-aliased pixel is an average of corner samples, and the occlusion starts from one primary ray's hit: take -n\n", argv[0]);
        return 1;
    }
    if (ao && (stereo == 3 || stereo == 4)) {
        fprintf(stderr, "%s: --ao with -m %s: %s: take -m s or -m o\n", argv[0], stereo == 3 ? "a" : "h",
                stereo == 3 ? "an anaglyph pixel has two primary rays, one an eye" : "a frame-packed image has no feature pass");
        return 1;
    }
    if (ao && gpus > 1) {
        fprintf(stderr, "%s: --ao with -g %d: the stage runs on the context that holds the whole frame; over several it is not built: take -g 1 (or -j)\n", argv[0], gpus);
        return 1;
    }
    if (ao && ssaa > 1) {
        fprintf(stderr, "%s: --ao with --ssaa %d: the occlusion is the plain frame's, not a supersampled one's: take one\n", argv[0], ssaa);
        return 1;
    }
    if (ao && (apng || png16)) {
        fprintf(stderr, "%s: --ao with %s: the shaded frame leaves as a PPM, --png, --jpeg, --exr or --raw: take one of those\n", argv[0],
                apng ? "--apng" : "--png16");
        return 1;
    }
    if (ao && (denoise || vdenoise)) {
        fprintf(stderr, "%s: --ao with %s: one stage stands between the render and the sink: take one\n", argv[0], denoise ? "--denoise" : "--vdenoise");
        return 1;
    }
    if (ao && depth_gpu) {
        fprintf(stderr, "%s: --ao with --depth gpu: no depth map is finished beside a shaded frame: take --exr -z, whose file carries it as Z\n", argv[0]);
        return 1;
    }
    if (ao && want_depth && !exr) {
        fprintf(stderr, "%s: --ao with -z: beside a shaded frame the depth map is the Z channel of the OpenEXR file only: it needs --exr\n", argv[0]);
        return 1;
    }
    if (denoise_tuned && !denoise) {
        fprintf(stderr, "%s: %s sets a weight of the denoiser: it needs --denoise\n", argv[0], denoise_tuned);
        return 1;
    }
    if (vdenoise_tuned && !vdenoise) {
        fprintf(stderr, "%s: %s sets a weight of the variance-guided denoiser: it needs --vdenoise\n", argv[0], vdenoise_tuned);
        return 1;
    }
    if (vdenoise && denoise) {
        fprintf(stderr, "%s: --vdenoise with --denoise: one stage stands between the render and the sink: take one\n", argv[0]);
        return 1;
    }
    /* what either denoiser is refused with, under the name of the one asked for */
    const char *dn = vdenoise ? "--vdenoise" : "--denoise";
    const int filtered = denoise || vdenoise;
    if (filtered && aa_depth >= 0) {
        fprintf(stderr, "%s: %s with -a: an anti-aliased pixel is an average of corner samples, and the denoiser's guides are one primary ray's: take -n\n", argv[0], dn);
        return 1;
    }
    if (filtered && stereo != 0) {
        fprintf(stderr, "%s: %s with -m %s: a stencil must not cross the seam between two eyes; that is not built: take -m m\n", argv[0], dn,
                stereo == 1 ? "s" : stereo == 2 ? "o" : stereo == 3 ? "a" : "h");
        return 1;
    }
    if (filtered && gpus > 1) {
        fprintf(stderr, "%s: %s with -g %d: a cyclic row shard has no neighbouring rows to filter over: take -g 1 (or -j)\n", argv[0], dn, gpus);
        return 1;
    }
    if (filtered && ssaa > 1) {
        fprintf(stderr, "%s: %s with --ssaa %d: the guides are the plain frame's, not a supersampled one's: take one\n", argv[0], dn, ssaa);
        return 1;
    }
    if (filtered && (apng || png16)) {
        fprintf(stderr, "%s: %s with %s: the denoised frame leaves as a PPM, --png, --jpeg, --exr or --raw: take one of those\n", argv[0], dn,
                apng ? "--apng" : "--png16");
        return 1;
    }
    if (filtered && want_depth) {
        fprintf(stderr, "%s: %s with -z: no depth map is made beside a denoised frame: take one\n", argv[0], dn);
        return 1;
    }
    if (filtered && exr_aov_given) {
        fprintf(stderr, "%s: %s with --exr-aov: the denoised file carries colour only: take one\n", argv[0], dn);
        return 1;
    }
    if (exr_pixel && !exr) {
        fprintf(stderr, "%s: --exr-pixel sets the OpenEXR file's sample type: it needs --exr\n", argv[0]);
        return 1;
    }
    if (exr_aov_given && !exr) {
        fprintf(stderr, "%s: --exr-aov adds channels to the OpenEXR file: it needs --exr\n", argv[0]);
        return 1;
    }
    if (exr_aov_given && aa_depth >= 0) {
        fprintf(stderr, "%s: --exr-aov with -a: an anti-aliased pixel is an average of corner samples, not one primary ray: no hit to record\n", argv[0]);
        return 1;
    }
    if (exr_aov_given && samples > 1) {
        fprintf(stderr, "%s: --exr-aov with -n %d: a pixel of several samples has no single primary ray: take -n 1\n", argv[0], samples);
        return 1;
    }
    if (exr_aov_given && (stereo == 3 || stereo == 4)) {
        fprintf(stderr, "%s: --exr-aov with -m %s: %s: take -m s or -m o\n", argv[0], stereo == 3 ? "a" : "h",
                stereo == 3 ? "an anaglyph pixel has two primary rays, one an eye" : "a frame-packed image has no feature channels");
        return 1;
    }
    if (exr && (png || jpeg || raw_path || png16 || apng)) {
        fprintf(stderr, "%s: --exr with %s: the OpenEXR file is the run's colour file; this one is not written beside it: take one\n", argv[0],
                png16 ? "--png16" : png ? "--png" : jpeg ? "--jpeg" : raw_path ? "--raw" : "--apng");
        return 1;
    }
    if (exr && (depth_gpu || depth_png)) {
        fprintf(stderr, "%s: --exr with %s: the map of -z is the file's Z channel as it is, in floats: it needs no finish\n", argv[0],
                depth_gpu ? "--depth gpu" : "--depth-png");
        return 1;
    }
    if (exr && gpus > 1) {
        fprintf(stderr, "%s: --exr with -g %d: the rows of several contexts are gathered as 8-bit pixels or doubles; a float gather is not built: take -g 1 (or -j)\n", argv[0], gpus);
        return 1;
    }
    if (apng_fps && !apng) {
        fprintf(stderr, "%s: --apng-fps sets the animated PNG's frame rate: it needs --apng\n", argv[0]);
        return 1;
    }
    if (apng && (png16 || png || jpeg || raw_path || want_depth)) {
        fprintf(stderr, "%s: --apng with %s: the animated PNG is the run's one colour file; this one is not written beside it: take one\n", argv[0],
                png16 ? "--png16" : png ? "--png" : jpeg ? "--jpeg" : raw_path ? "--raw" : "-z");
        return 1;
    }
    if (apng && (gpus > 1 || jobs > 1)) {
        fprintf(stderr, "%s: --apng with %s %d: the frames of an animated PNG meet one canvas on one GPU context, in order: take %s 1\n", argv[0],
                gpus > 1 ? "-g" : "-j", gpus > 1 ? gpus : jobs, gpus > 1 ? "-g" : "-j");
        return 1;
    }
    if (ssaa > 1 && aa_depth >= 0) {
        fprintf(stderr, "%s: --ssaa with -a: a frame is supersampled or anti-aliased recursively, not both: take one\n", argv[0]);
        return 1;
    }
    if (ssaa > 1 && stereo == 4) {
        fprintf(stderr, "%s: --ssaa with -m h: the 1080-line frame packing is not scalable: take -m s, o or a\n", argv[0]);
        return 1;
    }
    if (png16 && jpeg) {
        fprintf(stderr, "%s: --png16 with --jpeg: a JPEG has 8 bits a sample; --png16 needs --png --deflate gpu\n", argv[0]);
        return 1;
    }
    if (png16 && raw_path) {
        fprintf(stderr, "%s: --png16 keeps the doubles on the GPU and --raw brings them back: take one\n", argv[0]);
        return 1;
    }
    if (png16 && !(png && deflate_gpu)) {
        fprintf(stderr, "%s: --png16 has the GPU make the PNG file at 16 bits a sample: it needs --png --deflate gpu\n", argv[0]);
        return 1;
    }
    if (png16 && want_depth && !(depth_gpu && depth_png)) {
        fprintf(stderr, "%s: --png16 with -z: the map's 16-bit file is made on the GPU: it needs --depth gpu --depth-png\n", argv[0]);
        return 1;
    }
    if (png16 && gpus > 1) {
        fprintf(stderr, "%s: --png16 with -g %d: the rows of several contexts are gathered as 8-bit pixels; a 16-bit file is made by one context: take -g 1 (or -j)\n", argv[0], gpus);
        return 1;
    }
    if (deflate_gpu && !png) {
        fprintf(stderr, "%s: --deflate gpu compresses the PNG file: it needs --png\n", argv[0]);
        return 1;
    }
    if (jpeg && png) {
        fprintf(stderr, "%s: --jpeg and --png each name the frame's one image file: take one\n", argv[0]);
        return 1;
    }
    if (jpeg && raw_path) {
        fprintf(stderr, "%s: --jpeg has the GPU make the file from its 8-bit image and --raw brings doubles back: take one\n", argv[0]);
        return 1;
    }
    if (jpeg_quality && !jpeg) {
        fprintf(stderr, "%s: --jpeg-quality sets the JPEG file's quality: it needs --jpeg\n", argv[0]);
        return 1;
    }
    if (jpeg_sampling >= 0 && !jpeg) {
        fprintf(stderr, "%s: --jpeg-sampling sets the JPEG file's chroma sampling: it needs --jpeg\n", argv[0]);
        return 1;
    }
    if (jpeg && depth_gpu) {
        fprintf(stderr, "%s: --jpeg with --depth gpu: the device finishes the map beside a PNG or a PPM only; take --depth host with --jpeg\n", argv[0]);
        return 1;
    }
    if (depth_gpu && !want_depth) {
        fprintf(stderr, "%s: --depth gpu finishes the depth map of -z: it needs -z\n", argv[0]);
        return 1;
    }
    if (depth_gpu && raw_path) {
        fprintf(stderr, "%s: --depth gpu brings no doubles back and --raw dumps them: take --depth host with --raw\n", argv[0]);
        return 1;
    }
    if (depth_png && !(depth_gpu && png && deflate_gpu)) {
        fprintf(stderr, "%s: --depth-png has the GPU compress the map's PNG: it needs --depth gpu --png --deflate gpu\n", argv[0]);
        return 1;
    }
    int (*setup)(scene *, int, int, int, char *) = NULL;
    int (*frame_count)(int, char *) = NULL;
    int (*cleanup)(void) = NULL;
    if (!strcmp(scene_path, "builtin:yaml")) {
        /* the reference's scenes/yaml.c, built in: -u names the YAML file, one document per frame */
        setup = yaml_scene_setup;
        frame_count = yaml_scene_frames;
    } else {
        void *dl = dlopen(scene_path, RTLD_NOW);
        if (!dl) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        *(void **)(&setup) = dlsym(dl, "scene_setup");
        *(void **)(&frame_count) = dlsym(dl, "scene_frames");
        *(void **)(&cleanup) = dlsym(dl, "scene_cleanup");
    }
    if (!setup) { fprintf(stderr, "%s has no scene_setup\n", scene_path); return 1; }
    if (frame_count && !frames_given) frames = frame_count(dims, config);
    if (last < 0) last = frames - 1;
    register_objects(objects_dir);

    /* the one place where the flags become the frame request (the refusals above have sorted out what goes together).  The image
     * comes back in doubles only when something asks for them (--raw, a depth map of -z that the host finishes): the file of
     * --jpeg or --png --deflate gpu is then encoded from the host's bytes; otherwise the GPU quantises and 4 bytes a pixel come
     * back instead of 32, or only the file does */
    const int want_f64 = !exr && (raw_path != NULL || (want_depth && !depth_gpu));
    const ndt_colour_kind file_kind = jpeg ? NDT_COLOUR_JPEG : deflate_gpu ? NDT_COLOUR_PNG : NDT_COLOUR_F64;
    frame_request.width = width; frame_request.height = height; frame_request.samples = samples; frame_request.threads = threads;
    frame_request.aa_diff = aa_diff; frame_request.aa_depth = aa_depth; frame_request.stereo = stereo; frame_request.specular = specular;
    frame_request.max_optic_depth = depth; frame_request.ssaa = ssaa;
    frame_request.jpeg_quality = jpeg_quality; frame_request.jpeg_sampling = jpeg_sampling < 0 ? 0 : jpeg_sampling;
    frame_request.exr_pixel = exr_pixel;
    frame_request.exr_features = exr_aov;
    frame_request.denoise_iterations = denoise; frame_request.denoise_normal_power_log2 = denoise_normal;
    frame_request.denoise_sigma_colour = denoise_colour; frame_request.denoise_sigma_plane = denoise_plane;
    frame_request.sample_cap = sample_cap;
    frame_request.vdenoise_iterations = vdenoise; frame_request.vdenoise_normal_power_log2 = vdenoise_normal;
    frame_request.vdenoise_k_colour = vdenoise_colour; frame_request.vdenoise_sigma_plane = vdenoise_plane;
    frame_request.ao_samples = ao; frame_request.ao_radius = ao_radius; frame_request.ao_strength = ao_strength; frame_request.ao_seed = ao_seed;
    frame_request.colour = exr ? NDT_COLOUR_EXR : apng ? NDT_COLOUR_APNG : png16 ? NDT_COLOUR_PNG16 : want_f64 ? NDT_COLOUR_F64
                         : file_kind != NDT_COLOUR_F64 ? file_kind : NDT_COLOUR_RGBA8;
    frame_request.map = !want_depth ? NDT_MAP_NONE : exr ? NDT_MAP_EXR_Z : !depth_gpu ? NDT_MAP_F64 : png16 ? NDT_MAP_PNG16 : depth_png ? NDT_MAP_PNG : NDT_MAP_DEPTH8;
    job_opts.dims = dims; job_opts.raw_path = raw_path; job_opts.png = png;
    job_opts.host_file = want_f64 ? file_kind : NDT_COLOUR_F64;
    job_opts.gpus = gpus > 1 ? gpus : 1;
    job_opts.apng_fps = apng_fps ? apng_fps : 24;
    {
        const int upto = last < frames - 1 ? last : frames - 1, from = first > 0 ? first : 0;
        job_opts.apng_frames = upto >= from ? upto - from + 1 : 0;
    }
    ndt_render_fit_on_gpu(fit_gpu);
    ndt_render_kd_on_gpu(kd_gpu);
    if (job_opts.gpus > 1) {
        printf("one frame over %d GPU contexts (%d device(s) visible)\n", job_opts.gpus, ndt_hip_device_count());
        ndt_render_use_devices(job_opts.gpus);
    }
    /* -j K: K frames in flight.  The scene program runs on this thread, frame after frame (it may
     * keep state between frames, ndt.c:1818-1825); everything after it -- bounding spheres, kd-tree,
     * upload, render, image files -- happens on K worker threads, each with its own GPU context.
     * This is the reference's MPI_MODE_FRAME (rank 0 builds the scenes, the others render, ndt.c:1770-1830)
     * inside one process. */
    pthread_t *workers = NULL;
    if (jobs > 1 && !dump_path) {
        workers = (pthread_t *)calloc((size_t)jobs, sizeof(pthread_t));
        queue_cap = jobs;
        queue = (frame_job *)calloc((size_t)queue_cap, sizeof(frame_job));
        for (int k = 0; k < jobs; ++k) pthread_create(&workers[k], NULL, worker_main, (void *)(long)k);
    }
    double t_all = now_s();
    int rendered = 0;
    for (int i = 0; i < frames && i <= last; ++i) {
        scene *scn = (scene *)calloc(1, sizeof(scene));
        setup(scn, dims, i, frames, config);
        if (i < first) {            /* earlier frames still run scene_setup (ndt.c:1818-1825) */
            scene_free(scn);
            free(scn);
            continue;
        }
        printf("Scene has %i objects and %i lights\n", scn->num_objects, scn->num_lights);
        if (dump_path) {
            char err[256];
            ndt_flat_builder fb;
            /* --fit gpu, --kd gpu: the dump needs a device then; there is no falling back to the host */
            if (((fit_gpu || kd_gpu) ? ndt_flatten_scene_gpu(scn, &fb, err, sizeof(err), threads, fit_gpu, kd_gpu, NULL, NULL)
                                     : ndt_flatten_scene_mt(scn, &fb, err, sizeof(err), threads)) != 0) { fprintf(stderr, "%s\n", err); return 1; }
            if (i == last || i == frames - 1) ndt_write_ndtscene(&fb.fs, scn->name, dump_path);
            ndt_flat_builder_free(&fb);
            scene_free(scn);
            free(scn);
            continue;
        }
        ++rendered;
        if (workers) {
            queue_push(scn, i);
        } else {
            const int ok = render_frame(scn, i);
            scene_free(scn);
            free(scn);
            if (!ok) return 1;
        }
    }
    if (workers) {
        queue_close();
        for (int k = 0; k < jobs; ++k) pthread_join(workers[k], NULL);
        free(workers);
        if (worker_failed) return 1;
    }
    if (!apng_close()) return 1;
    if (rendered > 1) printf("%d frames in %.3fs (%.2f frames/s)\n", rendered, now_s() - t_all, rendered / (now_s() - t_all));
    if (cleanup) cleanup();
    return 0;
}
