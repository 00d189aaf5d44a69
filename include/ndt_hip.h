/*
 * ndt_hip.h -- C ABI of libndt_hip.so, the MI355X (gfx950) ray-trace core for ndt.
 *
 * This library replaces exactly one thing in the reference: the body of
 *     int render_image(scene *scn, char *name, ..., int width, int height, int samples,
 *                      stereo_mode mode, int threads, ..., int max_optic_depth, ...)
 * (reference ndt.c:900), i.e. the loop nest render_lines_thread (ndt.c:803) ->
 * render_line (ndt.c:735) -> render_pixel (ndt.c:578) -> get_pixel_color (ndt.c:456) ->
 * get_ray_color (ndt.c:329) / apply_lights (ndt.c:71) -> trace_kd (object.c:683) ->
 * kd_tree_intersect (kd-tree.c:570) -> trace (object.c:692) -> obj->intersect (objects/ *.c).
 *
 * The boundary is plain C: pointers, sizes, ints and doubles.  A scene crosses it as an
 * `ndt_flat_scene`: the reference's pointer-rich `scene` / `object` / `kd_tree_t` graph
 * flattened into index-linked arrays (INTEGRATION.md shows the ~150-line flattening stub a
 * maintainer adds next to render_image).  All reals are IEEE double, as in the reference.
 *
 * Error convention: every entry point returns 0 on success and a negative NDT_E_* code on
 * failure; ndt_hip_last_error() gives the message.  The reference's exit(1)-on-error habit
 * (object.c:233-236) is deliberately not carried into the library.
 */
#ifndef NDT_HIP_H
#define NDT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDT_HIP_ABI_VERSION 3

/* Dimensions the gfx950 kernels are instantiated for.  The reference accepts any N >= 3
 * (ndt.c:1450 `-d`); BASELINE.json's configs span 3..8. */
#define NDT_MIN_DIMS 3
#define NDT_MAX_DIMS 12
/* Lights of a scene.  The lighting kernels take them in windows of at most 64 (option "light_window"). */
#define NDT_MAX_LIGHTS 1024

#define NDT_OK              0
#define NDT_E_INVALID      -1   /* malformed scene / argument */
#define NDT_E_UNSUPPORTED  -2   /* valid for the reference, but not for the device path */
#define NDT_E_DEVICE       -3   /* HIP runtime failure */
#define NDT_E_NOMEM        -4   /* also: a device buffer of the context could not be allocated -- from ndt_hip_render*, the
                                   multi-context and async paths and ndt_hip_upload_scene too, which answered NDT_E_DEVICE before */
#define NDT_E_STATE        -5   /* call out of order (no scene uploaded, ...) */

/* Object kinds = the reference's built-in plugins (objects/ *.c `type_name`). */
enum ndt_object_type {
    NDT_OBJ_SPHERE    = 0,  /* objects/sphere.c    */
    NDT_OBJ_HPLANE    = 1,  /* objects/hplane.c    */
    NDT_OBJ_HDISK     = 2,  /* objects/hdisk.c     */
    NDT_OBJ_CYLINDER  = 3,  /* objects/cylinder.c  */
    NDT_OBJ_HCYLINDER = 4,  /* objects/hcylinder.c */
    NDT_OBJ_ORTHOTOPE = 5,  /* objects/orthotope.c */
    NDT_OBJ_HCUBE     = 6,  /* objects/hcube.c     */
    NDT_OBJ_HFACET    = 7,  /* objects/hfacet.c    */
    NDT_OBJ_FACET     = 8,  /* objects/facet.c     */
    NDT_OBJ_TYPE_COUNT = 9
};

/* Same numbering as the reference's light_type enum (scene.h:23-31). */
enum ndt_light_type {
    NDT_LIGHT_AMBIENT     = 0,
    NDT_LIGHT_POINT       = 1,
    NDT_LIGHT_DIRECTIONAL = 2,
    NDT_LIGHT_SPOT        = 3,
    NDT_LIGHT_DISK        = 4,  /* area lights: a random point of the disk / rectangle per shading evaluation */
    NDT_LIGHT_RECT        = 5   /* (ndt.c:116-147); rendered by the sampled path, parity is statistical */
};

/* One light (reference `light`, scene.h:36-49).  pos/dir are offsets, in doubles, into
 * ndt_flat_scene.vecs; -1 when the light has none. */
typedef struct ndt_flat_light {
    int32_t type;
    int32_t pos_off;
    int32_t dir_off;
    int32_t area_off;           /* ABI 3, DISK / RECT: u1[dims] then v1[dims] (scene_prepare_light, scene.c:182-195), else -1 */
    double  red, green, blue;
    double  angle;              /* spot cone half-angle, degrees (ndt.c:204) */
    double  radius;             /* ABI 3, DISK / RECT: the sample is pos + x*radius*u1 + y*radius*v1 (ndt.c:126-141) */
} ndt_flat_light;

/* One object (reference `object`, object.h:23-74) with its API-level parameters as the scene
 * wrote them (object_add_pos/dir/size/flag).  Ray-invariant data the plugins derive lazily in
 * their prepare() is recomputed inside the library.
 *
 * Objects [0, n_items) are the kd items in kd id order (kd-tree.c:448); the per-ray visit
 * mask (kd-tree.c:600) is indexed by that position.  Objects >= n_items are nested
 * primitives owned by a composite (`parent` >= 0): the orthotope faces an hcube builds in
 * add_faces (objects/hcube.c:34).  Clusters never appear: object_kdlist_add flattens them
 * (object.c:636-643). */
typedef struct ndt_flat_object {
    int32_t type;               /* enum ndt_object_type */
    int32_t transparent;        /* object.h:24 */
    int32_t parent;             /* -1 for kd items */
    int32_t n_pos,  pos_off;    /* pos[i] = vecs + pos_off + i*dims */
    int32_t n_dir,  dir_off;
    int32_t n_size, size_off;   /* into sizes[] */
    int32_t n_flag, flag_off;   /* into flags[] */
    int32_t n_obj,  obj_off;    /* children: obj_refs[obj_off .. obj_off+n_obj) are object indices */
    int32_t bounds_center_off;  /* into vecs[] */
    double  bounds_radius;      /* >0: gate with bounding sphere; <=0: no gate (object.c:618-624) */
    double  red, green, blue;
    double  red_r, green_r, blue_r;
    double  refract_index;
} ndt_flat_object;

/* One kd-tree node (reference kd_node_t, kd-tree.h:52-59).  Interior: dim >= 0, left/right
 * are node indices.  Leaf: dim < 0, items are leaf_refs[first .. first+num). */
typedef struct ndt_flat_kdnode {
    int32_t dim;
    int32_t num;
    int32_t left, right;
    int32_t first;
    int32_t _pad;
    double  boundary;
} ndt_flat_kdnode;

typedef struct ndt_flat_scene {
    int32_t abi_version;        /* NDT_HIP_ABI_VERSION */
    int32_t dims;

    /* pools */
    const double  *vecs;     int64_t n_vecs;      /* doubles */
    const double  *sizes;    int64_t n_sizes;
    const int32_t *flags;    int64_t n_flags;
    const int32_t *obj_refs; int64_t n_obj_refs;

    /* camera after camera_aim (camera.c:132), before render_image's dirX *= W/H (ndt.c:926);
     * offsets into vecs.  cam_type: 0 CAMERA_NORMAL (camera.c:557-575), 1 CAMERA_VR, 2 CAMERA_PANO (camera.c:506-555; they
     * need the ABI 2 fields below: fields of view, local axes). */
    int32_t cam_type;
    int32_t cam_pos_off, cam_img_orig_off, cam_dir_x_off, cam_dir_y_off;
    double  cam_focal_distance;

    /* scene colours: scn->ambient (scene.h:59) and bg_* (scene.h:60) */
    double ambient[3];
    double background[4];

    const ndt_flat_light  *lights;  int32_t n_lights;
    const ndt_flat_object *objects; int32_t n_objects; int32_t n_items;

    /* kd-tree (kd-tree.h:63-71): node 0 is the root */
    const ndt_flat_kdnode *kd_nodes;  int32_t n_kd_nodes;
    const int32_t         *leaf_refs; int32_t n_leaf_refs;   /* object indices (< n_items) */
    const int32_t         *inf_refs;  int32_t n_inf;         /* infinite objects, kd-tree.c:459 */
    int32_t bb_lower_off, bb_upper_off;                      /* root AABB, into vecs */

    /* ABI 2 -- the rest of the camera (camera.h:34-76), used by recursive anti-aliasing, stereo
     * modes and the VR / panorama cameras; offsets into vecs, -1 when the producer has none.
     * cam_aperture_radius != 0 makes recursive AA and samples>1 sample the lens (ndt.c:528-542: the reference's global
     * drand48 stream; here counter-based streams): such frames are stochastic renders, parity is statistical. */
    double  cam_aperture_radius;
    double  cam_h_fov, cam_v_fov;                            /* camera.h:52-53 */
    int32_t cam_left_eye_off, cam_right_eye_off;             /* camera.h:60-61 */
    int32_t cam_local_x_off, cam_local_y_off, cam_local_z_off;   /* camera.h:69-71 */
    int32_t _pad2;
} ndt_flat_scene;

/* Arguments of one render_image call (ndt.c:900).  Rows are dealt cyclically exactly like the
 * reference's threads/MPI_ROW split (ndt.c:812-820): this call renders image rows
 * j = row_begin, row_begin+row_step, ... < height, and output row k holds image row
 * row_begin + k*row_step.  row_begin=0,row_step=1 renders the whole frame. */
typedef struct ndt_render_params {
    int32_t width, height;
    int32_t max_optic_depth;    /* `-l`, default 128 (ndt.c:1413) */
    int32_t samples;            /* `-n`.  1 = the deterministic path.  > 1 = jittered samples + lens
                                 * sampling + the adaptive loop (ndt.c:470-568) with a per-(pixel, sample) counter-based
                                 * random stream: reproducible, independent of sharding, statistically equivalent to
                                 * the reference's drand48 stream; in every stereo mode, through every camera, with or
                                 * without a depth map (a pixel's depth is then its LAST sample's, ndt.c:362-373) */
    int32_t row_begin, row_step;
    int32_t specular;           /* 1 = specular_enabled (ndt.c:41) */
    int32_t profile;            /* 1 = bracket trace kernels with hipEvents (fills *_ms below) */
    /* ABI 2.  Whitted's recursive anti-aliasing (`-a diff,depth`; ndt.c:655-733, 1039-1087): the
     * first pass renders (width+1) x (height+1) corner samples, every output pixel is the average
     * of its four corners and is subdivided (5 new samples per level, up to aa_depth+1 levels)
     * while the corners differ by more than aa_diff/255.  The output is the resampled image
     * (width x height doubles; the reference quantises it to 8 bits when it stores it). */
    int32_t recursive_aa;       /* 0 = off */
    int32_t aa_diff;            /* reference default 20 (ndt.c:1412) */
    int32_t aa_depth;           /* reference default 4 (ndt.c:1411) */
    int32_t stereo;             /* ndt_stereo_mode (needs the eyes in the flat scene); with recursive_aa: every mode but HIDEF */
    int32_t reserved[4];        /* must be 0 */
} ndt_render_params;

typedef struct ndt_render_stats {
    /* rays actually traced on the device: one per unique trace_kd query */
    int64_t rays_primary, rays_secondary, rays_shadow;
    /* rays the reference executes for the same pixels: every pixel's ray tree times the
     * adaptive loop's repeat count k (ndt.c:488) */
    int64_t rays_ref_equiv;
    int32_t levels;             /* ray-tree depth reached */
    int32_t trace_launches;     /* launches of the trace kernel */
    double  trace_ms;           /* summed device time of those launches (profile=1) */
    double  frame_ms;           /* device time of the whole call (profile=1) */
    int64_t node_capacity;      /* ray-tree nodes the workspace holds */
    /* ABI 2 */
    int64_t pixels_resampled;   /* recursive AA: pixels that were subdivided (the reference's "pixels resampled") */
    int64_t aa_samples;         /* recursive AA: extra get_pixel_color samples rendered by the second pass;
                                 * stochastic renders (-n > 1, area lights): samples the adaptive loop consumed
                                 * (rays_* then also count the samples rendered ahead and dropped) */
} ndt_render_stats;

/* stereo_mode (ndt.c:46-48).  SIDE_SIDE / OVER_UNDER put the left-eye image in the left / top half and
 * the right-eye image in the other (each squeezed to half size), ANAGLYPH mixes the luminance of the
 * two eyes into red and blue (ndt.c:590-650).  HIDEF packs 1080 lines of the left eye, 45 black lines and 1080
 * lines of the right eye (ndt.c:614-631; `-m h` sets 1920x2205); the reference leaves the alpha of the black
 * lines unset, this library writes 1. */
enum ndt_stereo_mode {
    NDT_STEREO_MONO = 0, NDT_STEREO_SIDE_SIDE = 1, NDT_STEREO_OVER_UNDER = 2, NDT_STEREO_ANAGLYPH = 3, NDT_STEREO_HIDEF = 4
};

typedef struct ndt_hip_ctx ndt_hip_ctx;

/* Create a context on HIP device `device` with its own stream.  Fails with NDT_E_DEVICE when
 * no gfx950 device is usable -- there is no CPU fallback in this library. */
int ndt_hip_create(int device, ndt_hip_ctx **out);
int ndt_hip_destroy(ndt_hip_ctx *ctx);

/* Validate the scene, derive the plugins' prepare() data, lay it out for the device and copy
 * it to HBM.  Replaces the per-frame state render_image reads: `scn` and the global `kdtree`
 * (ndt.c:68). */
int ndt_hip_upload_scene(ndt_hip_ctx *ctx, const ndt_flat_scene *scene);

/* render_image (ndt.c:900) for the rows selected by `p`.  `rgba` receives
 * rows*width*4 doubles laid out like the reference's dbl image (image.c:126: r,g,b,a per
 * pixel, row-major).  _device: `rgba` is a device pointer on ctx's device (stays in HBM);
 * plain: `rgba` is host memory.  Both return when the frame is complete: every kernel of it has
 * finished on the context's stream (the last one posts a tag to host-mapped memory the call waits for),
 * so the image may be read from any stream or copied out at once. */
int ndt_hip_render_device(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, ndt_render_stats *stats);
int ndt_hip_render(ndt_hip_ctx *ctx, const ndt_render_params *p, double *rgba, ndt_render_stats *stats);

/* The same with the depth map render_image fills when it is given a depth file name (ndt.c:930-935,
 * 753-756): `depth` receives rows*width doubles, 1/distance of the primary hit (the left eye's for
 * ANAGLYPH), 0 where the primary ray misses.  With recursive_aa: the first pass's depths (ndt.c:930-935) -- but not beside
 * a stochastic anti-aliased render (a lens, area lights or samples > 1 under recursive_aa).  (The reference leaves the
 * previous pixel's value when the hit lies within EPSILON of the eye; this library writes 0.) */
int ndt_hip_render_depth_device(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, void *d_depth, ndt_render_stats *stats);
int ndt_hip_render_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, double *rgba, double *depth, ndt_render_stats *stats);

/* Batch of trace_kd queries (object.c:683) against the uploaded scene -- the unit the
 * known-answer tests pin.  o, v: n*dims doubles (ray-major); dist_limit: n doubles with the
 * reference's meaning (<0 closest hit, 0 any hit, >0 first hit within limit; ndt.c:177-189).
 * Outputs (host): obj[n] = object index or -1; hit, normal: n*dims doubles, zero when obj<0. */
int ndt_hip_trace_rays(ndt_hip_ctx *ctx, int64_t n, const double *o, const double *v,
                       const double *dist_limit, int32_t *obj, double *hit, double *normal);

/* bounds_list_optimal (bounding.c:177-240) for n_lists point lists at once, on ctx's device and stream: the minimum
 * enclosing sphere search (Nelder-Mead over the centre, seeded with the centroid) that object_get_bounds (object.c:582-603)
 * runs per object, and a frame runs per object and per nested hcube face before it can be uploaded.  List i is points
 * first[i] .. first[i+1] (first: n_lists + 1 entries, ascending) of points[.][dims] and point_radius[.], in the order
 * bounds_list_optimal walks the list (head first: bounds_list_add prepends).  centers: n_lists x dims, radii: n_lists,
 * exactly what bounds_list_optimal returns -- object_get_bounds's `+ EPSILON` stays with the caller.
 * Bit-identical to the host fit.  NDT_E_INVALID: dims outside 3..12, an empty list, a non-finite input
 * (the caller fits those itself).  Synchronous.  No scene has to be uploaded; the device buffers belong to the context
 * and are reused by the next call. */
int ndt_hip_fit_spheres(ndt_hip_ctx *ctx, int32_t dims, int64_t n_lists, const int64_t *first,
                        const double *points, const double *point_radius,
                        double *centers, double *radii);
/* Kernel launches the context's last ndt_hip_fit_spheres call made (one per group of list lengths; 0 for an empty batch). */
int ndt_hip_fit_launches(ndt_hip_ctx *ctx);

/* kd_tree_build (kd-tree.c:421-477) for the item boxes of a frame, on ctx's device and stream: the exhaustive split search of
 * kd_tree_split_node (kd-tree.c:294-419) level by level, every candidate of every open node scored at once.  Input: the boxes
 * object_kdlist_add makes (object.c:633-681), lower / upper: n_items x dims, and one byte per item, finite != 0 for the
 * reference's `bounds.radius >= 0` (kd-tree.c:448-463).  Inverted boxes (lower = DBL_MAX, upper = -DBL_MAX) are legal and go
 * through the search's own comparisons.  The tree is the host builder's, byte for byte, in the arrays an ndt_flat_scene
 * carries: nodes in preorder (left = node + 1; a leaf's items are leaf_refs[first .. first + num), in list order), inf_refs
 * (the other items, ascending) and the root box (DBL_MAX / -DBL_MAX without a finite item).  No item, or no finite one: one
 * empty leaf.
 * Two calls, because the tree's size is not known in advance: the build leaves the tree in the context and fills *counts;
 * the fetch copies it into arrays of those sizes (nodes: n_kd_nodes, leaf_refs: n_leaf_refs, inf_refs: n_inf, bb_*: dims).
 * The tree stays fetchable until the context's next build.  Synchronous.  No scene has to be uploaded.
 * Device buffers belong to the context, only grow and are reused.  Growth policy: a level's node, reference and candidate
 * counts are known before anything of it is written; a buffer that is too small becomes max(what is needed, twice its size),
 * its contents moved, and nothing is ever written past a buffer.  Upper bound: 2^30 item references over all nodes of the
 * tree under construction (4 GiB), 2^26 nodes; beyond that, or when the device has no such memory, NDT_E_NOMEM with the size
 * that was needed -- never a partial tree.
 * NDT_E_INVALID, before any device call: dims outside 3..12, n_items < 0, a NULL array or context, a NaN bound (the caller
 * builds those itself).  NDT_E_UNSUPPORTED: the tree is deeper than the traversal stack of the trace kernels holds (40 levels;
 * the upload refuses such a tree as well). */
typedef struct ndt_kd_counts {
    int32_t n_kd_nodes, n_leaf_refs, n_inf;
    int32_t depth;              /* levels of the tree: 1 for a single leaf */
    int32_t launches;           /* kernel launches of the build: at most three a level */
    int32_t grows;              /* device buffers that had to be replaced by larger ones during the build */
} ndt_kd_counts;
int ndt_hip_build_kdtree(ndt_hip_ctx *ctx, int32_t dims, int32_t n_items, const double *lower, const double *upper,
                         const uint8_t *finite, ndt_kd_counts *counts);
int ndt_hip_kdtree_fetch(ndt_hip_ctx *ctx, ndt_flat_kdnode *nodes, int32_t *leaf_refs, int32_t *inf_refs,
                         double *bb_lower, double *bb_upper);
/* Kernel launches the context's last build made. */
int ndt_hip_kd_launches(ndt_hip_ctx *ctx);

/* Quantise a double image like the reference does at save time: pixel_d2c (image.h:36-39),
 * (unsigned char)(sqrt(clamp01(x))*255) per channel.  d_rgba: device, n_pixels*4 doubles;
 * d_rgba8: device, n_pixels*4 bytes. */
int ndt_hip_quantize_device(ndt_hip_ctx *ctx, const void *d_rgba, void *d_rgba8, int64_t n_pixels);

/* What the calls that deliver a finished image write: the double framebuffer (4 doubles per pixel, image.c:126) or the
 * bytes the reference stores at save time (pixel_d2c on every channel, image.h:36-39, image.c:648-651: 4 bytes per pixel). */
enum ndt_image_format { NDT_IMAGE_F64 = 0, NDT_IMAGE_RGBA8 = 1 };

/* render_image followed by the reference's save-time quantisation, on the device: `rgba8` (host) receives
 * rows*width*4 bytes.  An eighth of ndt_hip_render's bytes cross PCIe. */
int ndt_hip_render_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *rgba8, ndt_render_stats *stats);

/* The same without waiting for the bytes to arrive: the call returns when the frame is complete in HBM and quantised; its copy to
 * `rgba8` -- pinned host memory -- runs on a copy stream behind the NEXT call's rendering.  When a call returns, every EARLIER
 * frame of the context has arrived in its buffer; the frame of the call itself has when the next call, or
 * ndt_hip_render_rgba8_wait, returns -- until then `rgba8` must stay valid and is not to be read.  What "rendering took"
 * (ndt.c:978-984: pixels in host memory) costs per frame of a sequence is then the render. */
int ndt_hip_render_rgba8_async(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *rgba8, ndt_render_stats *stats);
int ndt_hip_render_rgba8_wait(ndt_hip_ctx *ctx);

/* The frame's image file made on the device: a complete, standard PNG (8-bit RGBA, one IDAT, no interlace) of the quantised
 * image, delivered into host memory -- what crosses PCIe is the file, not the image.  Every scanline is filtered with
 * filter 0 (None), 1 (Sub) or 2 (Up), whichever has the smallest sum of |filtered byte taken as int8| (ties to the lower
 * number; the first row has zeros above it); the filtered stream is deflated in independent chunks of 32 KiB, each with
 * distance-1 matches and a dynamic Huffman code of its own, each ending on a byte boundary; a chunk that would not shrink is
 * stored, which bounds the file.  The same image gives the same bytes.
 *   ndt_hip_png_bound          host arithmetic: the largest file the encoder can produce for width x rows; < 0 (NDT_E_INVALID)
 *                              for a size it does not take
 *   ndt_hip_encode_png_device  d_rgba8: width * rows * 4 bytes in the context's device memory
 *   ndt_hip_encode_png         rgba8: the same in host memory (uploaded first)
 *   ndt_hip_render_png         ndt_hip_render_rgba8 with the encoder in place of the download: every mode of it (-a, -n, stereo,
 *                              row shards: the PNG's height is the shard's row count)
 * `png` (host) receives the file, `cap` is its room.  NDT_E_INVALID: a NULL pointer, width < 1 or rows < 1, a size whose
 * filtered stream rows * (1 + 4 * width) exceeds 2^31 - 1 bytes.  NDT_E_NOMEM: `cap` is smaller than the file -- the error text
 * and stats->png_bytes carry the size needed and nothing is written to `png`.  The two encode calls need no scene.  Device
 * buffers belong to the context, only grow and are reused.  The calls return when the file is complete.
 * stats (may be NULL): idat_bytes = the zlib stream (header and Adler-32 included), chunks / chunks_stored = 32 KiB chunks in
 * all / left uncompressed, launches = kernel launches, rows_filter[f] = scanlines filtered with f, encode_ms = host time of the
 * encoder (launch to the file in host memory; the render of ndt_hip_render_png is not in it). */
typedef struct ndt_png_stats {
    int64_t png_bytes, idat_bytes;
    int32_t chunks, chunks_stored, launches;
    int32_t rows_filter[3];
    double encode_ms;
} ndt_png_stats;
int64_t ndt_hip_png_bound(int32_t width, int32_t rows);
int ndt_hip_encode_png_device(ndt_hip_ctx *ctx, const void *d_rgba8, int32_t width, int32_t rows, uint8_t *png, int64_t cap,
                              ndt_png_stats *stats);
int ndt_hip_encode_png(ndt_hip_ctx *ctx, const uint8_t *rgba8, int32_t width, int32_t rows, uint8_t *png, int64_t cap,
                       ndt_png_stats *stats);
int ndt_hip_render_png(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                       ndt_render_stats *render_stats);

/* The frame's image file as a JPEG made on the device: a complete baseline JFIF file (SOF0, 8 bit, Y Cb Cr) of the quantised
 * image, alpha ignored -- what the reference's libjpeg writer saves (image.c:346-412), in libjpeg's integer arithmetic: its
 * colour transform, its 4:2:0 averaging, its slow integer DCT, its quantiser, the Annex K tables scaled by `quality` the way
 * jpeg_set_quality does, the Annex K.3 Huffman tables.  Segments: SOI, APP0 (JFIF 1.01), DQT 0, DQT 1, SOF0, DHT x 4, DRI, SOS,
 * the scan, EOI.  One restart interval per MCU row (16 x 16 pixels under 4:2:0, 8 x 8 under 4:4:4): every interval is coded on
 * its own, RSTm between them.  Edges as libjpeg pads them.  The same image and parameters give the same
 * bytes -- the bytes libjpeg writes for them with restart_in_rows = 1.
 *   ndt_hip_jpeg_bound          host arithmetic: the largest file the encoder can produce; < 0 (NDT_E_INVALID) for a size or
 *                               parameters it does not take
 *   ndt_hip_encode_jpeg_device  d_rgba8: width * rows * 4 bytes in the context's device memory
 *   ndt_hip_encode_jpeg         rgba8: the same in host memory (uploaded first)
 *   ndt_hip_render_jpeg         ndt_hip_render_rgba8 with the encoder in place of the download: every mode of it (-a, -n, stereo,
 *                               row shards: the file's height is the shard's row count)
 * jp == NULL: the defaults (quality 95, 4:2:0).  `jpg` (host) receives the file, `cap` is its room.  NDT_E_INVALID, before
 * any device call: a NULL pointer, width < 1 or rows < 1, a dimension above 65535 (SOF0's limit), a quality outside 0 .. 100,
 * a sampling outside 0 .. 1, a reserved word that is not 0.  NDT_E_NOMEM: `cap` is smaller than the file -- the error text and
 * stats->jpeg_bytes carry the size needed and nothing is written to `jpg`.  The two encode calls need no scene.  Device buffers
 * belong to the context, only grow and are reused.  The calls return when the file is complete; none falls back.
 * stats (may be NULL): scan_bytes = what lies between SOS and EOI (stuffing and RSTm included), stuffed_bytes = the 0x00 bytes
 * put behind 0xFF, mcus / intervals = MCUs and restart intervals, launches = kernel launches, passes_max = the most passes an
 * interval took through the entropy coder's LDS bit buffer, encode_ms = host time of the encoder (launch to the file in host
 * memory; the render of ndt_hip_render_jpeg is not in it). */
typedef struct ndt_jpeg_params {
    int32_t quality;        /* 1 .. 100; 0 = 95 */
    int32_t sampling;       /* 0 = 4:2:0, 1 = 4:4:4 */
    int32_t reserved[2];    /* must be 0 */
} ndt_jpeg_params;
typedef struct ndt_jpeg_stats {
    int64_t jpeg_bytes, scan_bytes, stuffed_bytes;
    int32_t mcus, intervals, launches, passes_max;
    double encode_ms;
} ndt_jpeg_stats;
int64_t ndt_hip_jpeg_bound(int32_t width, int32_t rows, const ndt_jpeg_params *jp);
int ndt_hip_encode_jpeg_device(ndt_hip_ctx *ctx, const void *d_rgba8, int32_t width, int32_t rows, const ndt_jpeg_params *jp,
                               uint8_t *jpg, int64_t cap, ndt_jpeg_stats *stats);
int ndt_hip_encode_jpeg(ndt_hip_ctx *ctx, const uint8_t *rgba8, int32_t width, int32_t rows, const ndt_jpeg_params *jp, uint8_t *jpg,
                        int64_t cap, ndt_jpeg_stats *stats);
int ndt_hip_render_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_jpeg_params *jp, uint8_t *jpg, int64_t cap,
                        ndt_jpeg_stats *stats, ndt_render_stats *render_stats);

/* The depth map of `-z` finished on the device: what the reference does to the map before it saves it (ndt.c:1010-1016:
 * dbl_image_normalize, image.c:1025-1065, stretches it to 0 .. 1; the grey image v, v, v, 1 is then quantised with pixel_d2c
 * like every image).  With lo / hi the map's minimum / maximum, pixel i becomes the four bytes g, g, g, 255 with
 * g = pixel_d2c(hi > lo ? (d[i] - lo) / (hi - lo) : 0.0) -- bit for bit the host's arithmetic.
 *   ndt_hip_depth_rgba8_device   d_depth: n_pixels doubles in the context's device memory; d_rgba8: n_pixels * 4 bytes there.
 *                                Two kernel launches: a reduction to one {lo, hi} record per workgroup, and a kernel whose
 *                                workgroups each fold those records and then write their share of the pixels.
 *                                range_out (host, may be NULL) receives lo, hi.  Synchronous.  No scene has to be uploaded.
 *                                NDT_E_INVALID: a NULL pointer, n_pixels < 1, a misaligned pointer.  NDT_E_UNSUPPORTED: the map
 *                                holds a NaN or an infinity -- the error text names the lowest such pixel, and d_rgba8 is
 *                                not written (the reference's loop would give a range that depends on where the NaN sits).
 *   ndt_hip_render_rgba8_depth   ndt_hip_render_depth_device into the context's buffers, the image quantised and the map finished
 *                                there: rgba8 and depth8 (host) receive rows*width*4 bytes each -- 8 bytes a pixel cross PCIe
 *                                where ndt_hip_render_depth moves 40.  Accepts and refuses what ndt_hip_render_depth does.
 *   ndt_hip_render_png_depth     the same with ndt_hip_encode_png_device in place of the downloads.  The image always leaves as
 *                                a file (png, cap); the map as a file (depth_png, depth_cap) or as its bytes (depth8): exactly
 *                                one of depth_png / depth8 is not NULL.  stats (may be NULL): two records, [0] the image's
 *                                file, [1] the map's.  A buffer that is too small: NDT_E_NOMEM with the size needed in the
 *                                error text and in its stats record, and nothing written to that buffer (the image's file is
 *                                made first: it has arrived when only depth_cap is short).
 *   ndt_hip_depth_launches / ndt_hip_depth_ms   kernel launches of the context's last map (2), and the host time they took,
 *                                launch to the range in host memory. */
int ndt_hip_depth_rgba8_device(ndt_hip_ctx *ctx, const void *d_depth, int64_t n_pixels, void *d_rgba8, double *range_out);
int ndt_hip_render_rgba8_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *rgba8, uint8_t *depth8, double *range_out,
                               ndt_render_stats *stats);
int ndt_hip_render_png_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *png, int64_t cap, uint8_t *depth_png,
                             int64_t depth_cap, uint8_t *depth8, ndt_png_stats *stats, double *range_out,
                             ndt_render_stats *render_stats);
int ndt_hip_depth_launches(ndt_hip_ctx *ctx);
double ndt_hip_depth_ms(ndt_hip_ctx *ctx);

/* Regular K x K supersampling with a box filter in linear light, on the device (`ndt_hip --ssaa K`).  The ssaa frame of size
 * W x H is the frame of size K W x K H of the same scene and camera averaged over K x K blocks in doubles: sub-sample (a, b) of
 * output pixel (i, j) is pixel (K i + b, K j + a) of the large frame -- sub-sample (0, 0) is the plain frame's own sample -- and,
 * per channel, alpha included,
 *     out = (((s[0][0] + s[0][1]) + ... + s[0][K-1]) + s[1][0] + ... + s[K-1][K-1]) / (double)(K * K)
 * summed strictly left to right, sub-row a outer, sub-column b inner.  The 8-bit image is pixel_d2c of that.  The depth map of
 * an ssaa frame is the depth of sub-sample (0, 0): the plain W x H frame's map, not an average.  K = 1 is the plain frame.
 * Sub-row a of the output rows of a shard (row_begin b, row_step S) is the cyclic shard row_begin K b + a, row_step K S of the
 * large frame: a frame is K renders of ndt_hip_render_depth_device -- either pipeline; samples > 1 included, whose streams are
 * functions of the pixel id -- each folded into the accumulator by one kernel launch.  Memory: a frame K times as wide, not
 * K * K times as large; the buffers belong to the context, only grow and are reused.
 *   ndt_hip_ssaa_fold_device     one fold step on device buffers: d_pass = rows x K width_out x 4 doubles (sub-row a of the
 *                                rows), d_acc = rows x width_out x 4 doubles.  a = 0 writes d_acc, a > 0 adds to it, a = K - 1
 *                                then divides by K * K and, with d_rgba8 not NULL, writes rows x width_out x 4 bytes there
 *                                (earlier steps leave d_rgba8 alone).  d_pass and d_acc aligned to 16 bytes.  Synchronous.
 *                                No scene has to be uploaded.
 *   ndt_hip_render_ssaa_device   the whole frame into d_rgba (device, rows x width x 4 doubles, aligned to 16 bytes) and, when
 *                                d_depth is not NULL, the map into d_depth (rows x width doubles).  stats sums the K passes;
 *                                rays_ref_equiv is that of the K W x K H frame.
 *   ndt_hip_render_ssaa          the same into host memory (depth may be NULL)
 *   ndt_hip_render_ssaa_rgba8 / _png / _jpeg   the same frame as its bytes (written by the last fold), or through
 *                                ndt_hip_encode_png_device / ndt_hip_encode_jpeg_device as a file
 *   ndt_hip_render_ssaa_rgba8_depth   the bytes and the map finished by ndt_hip_depth_rgba8_device
 *   ndt_hip_ssaa_launches / ndt_hip_ssaa_ms   fold launches of the context's last ssaa frame (K; 0 for K = 1), and their summed
 *                                device time
 * NDT_E_INVALID with the cause in the error text, before any device work and with nothing written: K outside 1 .. 8,
 * recursive_aa set, NDT_STEREO_HIDEF (its 1080-line packing is not scalable), K * width or K * height beyond INT32_MAX, a NULL
 * pointer, an odd width side by side or an odd height over/under (the halves would not line up with the large frame's).
 * Everything else is accepted and refused as ndt_hip_render_depth_device does for the large frame.  There is no fallback. */
int ndt_hip_ssaa_fold_device(ndt_hip_ctx *ctx, const void *d_pass, void *d_acc, int32_t width_out, int32_t rows, int32_t K, int32_t a,
                             void *d_rgba8);
int ndt_hip_render_ssaa_device(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, void *d_rgba, void *d_depth, ndt_render_stats *stats);
int ndt_hip_render_ssaa(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, double *rgba, double *depth, ndt_render_stats *stats);
int ndt_hip_render_ssaa_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *rgba8, ndt_render_stats *stats);
int ndt_hip_render_ssaa_png(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                            ndt_render_stats *render_stats);
int ndt_hip_render_ssaa_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, const ndt_jpeg_params *jp, uint8_t *jpg, int64_t cap,
                             ndt_jpeg_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_render_ssaa_rgba8_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *rgba8, uint8_t *depth8, double *range_out,
                                    ndt_render_stats *stats);
int ndt_hip_ssaa_launches(ndt_hip_ctx *ctx);
double ndt_hip_ssaa_ms(ndt_hip_ctx *ctx);

/* 16 bits a sample (`ndt_hip --png16`): the frame and its depth map as PNG files of bit depth 16, made on the device from the
 * double framebuffer -- every other file passes through pixel_d2c's 256 levels.  A sample is
 *     q16(x) = (uint16_t)(sqrt(m) * 65535),   m = x clamped to 0 .. 1 by pixel_d2c's two comparisons in their order,
 * stored most significant byte first, as the file has it.  The colour file is colour type 6 (RGBA, 8 bytes a pixel), the
 * map's colour type 0 (grey, 2 bytes a pixel) with the value q16(hi > lo ? (d - lo) / (hi - lo) : 0.0) of
 * ndt_hip_depth_rgba8_device's lo / hi.  One IDAT, no interlace.  The row heuristic is the 8-bit file's with the pixel's width as
 * a parameter (Sub looks 8 or 2 bytes to the left; row stride 1 + 8 * width or 1 + 2 * width), and the deflate, assemble and
 * place kernels are the 8-bit file's own: the same image gives the same bytes.
 *   ndt_hip_quantize16_device    d_rgba: n_pixels * 4 doubles (device, aligned to 16 bytes); d_rgba16: n_pixels * 8 bytes (device,
 *                                aligned to 8): q16 of every channel in file byte order.  One launch, on the context's stream;
 *                                not synchronised, like ndt_hip_quantize_device.
 *   ndt_hip_depth_grey16_device  ndt_hip_depth_rgba8_device with one grey sample a pixel: d_grey16 = n_pixels * 2 bytes (device,
 *                                aligned to 4).  The same two launches, range and refusal of a NaN or an infinity.
 *   ndt_hip_png16_bound          the largest file for width x rows with channels = 4 (RGBA) or 1 (grey); < 0 (NDT_E_INVALID) for
 *                                other channel counts and for a size the encoder does not take: the 8-bit limit (a filtered
 *                                stream of at most 2^31 - 1 bytes) with this stride
 *   ndt_hip_encode_png16_device / ndt_hip_encode_png16   the file of width * rows * channels samples in file byte order, in the
 *                                context's device memory (aligned to the pixel: 8 or 2 bytes) or in host memory.  Errors and
 *                                stats are those of ndt_hip_encode_png_device / ndt_hip_encode_png.  No scene is needed.
 *   ndt_hip_render_png16         ndt_hip_render_device, ndt_hip_quantize16_device and the encoder: every mode of ndt_hip_render_png
 *   ndt_hip_render_png16_depth   ndt_hip_render_png_depth with both files at 16 bits; stats: two records.  Accepts and refuses
 *                                what ndt_hip_render_depth does
 *   ndt_hip_render_ssaa_png16 / _png16_depth   the same for the ssaa frame: q16 of the finished accumulator (one launch behind
 *                                the last fold) and, for the map, of sub-sample (0, 0)'s
 * Device buffers belong to the context, only grow and are reused.  The calls return when the file is in host memory.  None falls
 * back. */
int ndt_hip_quantize16_device(ndt_hip_ctx *ctx, const void *d_rgba, void *d_rgba16, int64_t n_pixels);
int ndt_hip_depth_grey16_device(ndt_hip_ctx *ctx, const void *d_depth, int64_t n_pixels, void *d_grey16, double *range_out);
int64_t ndt_hip_png16_bound(int32_t width, int32_t rows, int32_t channels);
int ndt_hip_encode_png16_device(ndt_hip_ctx *ctx, const void *d_samples, int32_t width, int32_t rows, int32_t channels, uint8_t *png,
                                int64_t cap, ndt_png_stats *stats);
int ndt_hip_encode_png16(ndt_hip_ctx *ctx, const uint8_t *samples, int32_t width, int32_t rows, int32_t channels, uint8_t *png,
                         int64_t cap, ndt_png_stats *stats);
int ndt_hip_render_png16(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                         ndt_render_stats *render_stats);
int ndt_hip_render_png16_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, uint8_t *png, int64_t cap, uint8_t *depth_png,
                               int64_t depth_cap, ndt_png_stats *stats, double *range_out, ndt_render_stats *render_stats);
int ndt_hip_render_ssaa_png16(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *png, int64_t cap, ndt_png_stats *stats,
                              ndt_render_stats *render_stats);
int ndt_hip_render_ssaa_png16_depth(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, uint8_t *png, int64_t cap, uint8_t *depth_png,
                                    int64_t depth_cap, ndt_png_stats *stats, double *range_out, ndt_render_stats *render_stats);

/* A frame sequence as ONE animated PNG (APNG; `ndt_hip --apng`), the difference between consecutive frames found on the device.
 * The file is 8-bit RGBA: signature, IHDR, acTL, then per frame an fcTL and one IDAT (frame 0, the default image, the whole
 * canvas) or one fdAT (every later frame: a sub-rectangle with a zlib stream of its own, made by the encoder of the still files
 * run on the smaller image), then IEND.  Sequence numbers run 0, 1, 2 ... over fcTL and fdAT together; every frame has dispose
 * NONE and the delay given at `begin`.  The canvas -- the previous frame -- stays in the context's device memory, and a later
 * frame is planned there against it:
 *   changed     a pixel whose 32-bit word differs from the canvas's
 *   rectangle   the tight bounding box of the changed pixels; nothing changed: the 1 x 1 pixel at (0, 0), blend SOURCE
 *   blend OVER (1)    when every changed pixel has alpha 255: the unchanged pixels inside the rectangle are sent as 00 00 00 00
 *               (alpha 0 keeps the canvas, alpha 255 replaces it: the decoded frame is exact)
 *   blend SOURCE (0)  otherwise: the rectangle's pixels as they are
 * What crosses PCIe per frame is the plan record and the rectangle's zlib stream.
 *   ndt_hip_apng_bound   host arithmetic: the most bytes one `add` can append for a width x rows canvas; < 0 (NDT_E_INVALID) exactly
 *                        where ndt_hip_png_bound is
 *   ndt_hip_apng_begin   opens the context's session (one at a time; a session still open is dropped): n_frames >= 1 frames are
 *                        to come -- acTL precedes them, so the count is fixed here --, each shown delay_num / delay_den seconds
 *                        (0 .. 65535 over 1 .. 65535), the animation played n_plays >= 0 times (0: for ever).  No device work
 *   ndt_hip_apng_add_device / ndt_hip_apng_add   the next frame, width * rows * 4 bytes in the context's device memory (aligned
 *                        to 4) or in host memory.  `out` receives exactly the bytes to append to the file; the first call's
 *                        start with the signature, IHDR and acTL.  Frame 0 takes a device-to-device copy into the canvas and
 *                        the encoder's 4 launches, a later frame 7 launches
 *   ndt_hip_render_apng_frame   renders the uploaded scene's shard and adds it from device memory: the 8-bit image never reaches
 *                        the host.  The shard's width and rows must be the session's.  ssaa 1: the plain frame, every mode of
 *                        ndt_hip_render_rgba8; ssaa 2 .. 8: the supersampled frame, with the refusals of ndt_hip_render_ssaa_rgba8
 *   ndt_hip_apng_end     after the n_frames-th frame: IEND into `out`, its length into *bytes; closes the session
 * NDT_E_INVALID, before any device work and with the cause in the error text: a NULL pointer, a size < 1, n_frames < 1,
 * delay_den < 1, a delay beyond 65535, no session open, a device pointer off its 4-byte pixels, one `add` more than n_frames,
 * `end` before the n_frames-th frame (the session stays open).  NDT_E_NOMEM: `cap` is smaller than what is to be appended; the
 * text and stats->bytes carry the size needed and nothing is written to `out`.  Any error from an `add` closes the session.
 * stats (may be NULL): frame = its index, bytes = appended, zlib_bytes = the zlib stream's, x y w h blend = its fcTL's,
 * changed / translucent = pixels that differ from the canvas / ... and have an alpha other than 255 (frame 0: 0 and 0),
 * launches = kernel launches, encode_ms = host time of the call without the render.  None of the calls falls back. */
typedef struct ndt_apng_stats {
    int64_t bytes, zlib_bytes, changed, translucent;
    int32_t frame, x, y, w, h, blend, launches, reserved;
    double encode_ms;
} ndt_apng_stats;
int64_t ndt_hip_apng_bound(int32_t width, int32_t rows);
int ndt_hip_apng_begin(ndt_hip_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, int32_t delay_num, int32_t delay_den,
                       int32_t n_plays);
int ndt_hip_apng_add_device(ndt_hip_ctx *ctx, const void *d_rgba8, uint8_t *out, int64_t cap, ndt_apng_stats *stats);
int ndt_hip_apng_add(ndt_hip_ctx *ctx, const uint8_t *rgba8, uint8_t *out, int64_t cap, ndt_apng_stats *stats);
int ndt_hip_render_apng_frame(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t ssaa, uint8_t *out, int64_t cap,
                              ndt_apng_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_apng_end(ndt_hip_ctx *ctx, uint8_t *out, int64_t cap, int64_t *bytes);

/* The frame as an OpenEXR file made on the device (`ndt_hip --exr`): the double framebuffer as it is, in linear light -- no clamp to
 * 0 .. 1 and no square root, which every other file passes through -- and the depth map of `-z` unstretched, as a channel of the
 * same file.  A single-part scanline file of version 2, little-endian: magic 76 2f 31 01, version word 2, the attributes channels,
 * compression (3: ZIP, 16 scanlines a block), dataWindow and displayWindow (0, 0, width - 1, rows - 1), lineOrder (0),
 * pixelAspectRatio (1), screenWindowCenter (0, 0), screenWindowWidth (1); one uint64 file offset per block; the blocks in order,
 * each int32 y of its first line, int32 dataSize, data.  Channels in the file's (alphabetical) order: A B G R, all HALF or all
 * FLOAT by ndt_exr_params, and Z, always FLOAT, when a map is given.
 *   FLOAT   (float)x, to nearest even (a double beyond the float range becomes an infinity, as the conversion defines)
 *   HALF    x clamped to +-65504, then rounded directly to binary16, to nearest even -- not through float, which rounds twice;
 *           no infinity is written, and a NaN becomes 0x7e00
 * A block's raw bytes are, per scanline, per channel in that order, `width` samples.  They are compressed as the format defines:
 * the even bytes, then the odd ones; the delta predictor out[i] = T[i] - T[i-1] + 128; one zlib stream a block, made by the
 * deflate of the PNG files (independent 32 KiB chunks, a dynamic Huffman code a chunk) with its matches at distance 2, the period
 * the two byte planes give equal float samples (equal half samples are runs of one byte, which that matches too).  A block whose
 * stream is not shorter than its raw bytes holds the raw bytes (dataSize = their count): the format's own rule.
 *   ndt_hip_exr_bound          the largest file for width x rows (host arithmetic: every block raw); < 0 (NDT_E_INVALID) for a bad
 *                              pixel type, a size below 1 or raw bytes beyond 2^31 - 1
 *   ndt_hip_encode_exr_device  the file of rows x width x 4 doubles (R G B A) and, when d_depth is not NULL, rows x width doubles
 *                              of map, both in the context's device memory, aligned to 8 bytes.  4 kernel launches; the host
 *                              reads an info record, then exactly the file's bytes.  No scene is needed
 *   ndt_hip_encode_exr         the same from host memory
 *   ndt_hip_render_exr         ndt_hip_render_device (with_depth: ndt_hip_render_depth_device) and the encoder: recursive_aa,
 *                              samples and stereo are just another double framebuffer; a row shard gives the file of its rows
 *   ndt_hip_render_ssaa_exr    the same for the frame supersampled K x K (ndt_hip_render_ssaa_device; Z is sub-sample (0, 0)'s)
 * ep may be NULL (half).  NDT_E_INVALID: a NULL pointer, a pixel type other than 0, 1, 2, a size below 1, a pointer off its
 * doubles.  NDT_E_NOMEM: `cap` is below the file; stats->file_bytes and the error text carry the size needed and nothing is
 * written to `out`.  stats (may be NULL): file_bytes, raw_bytes = the samples' bytes, blocks, blocks_raw = blocks that fell back
 * to raw bytes, launches, ms = host time of the encoder.  Device buffers belong to the context, only grow and are reused.  None
 * falls back. */
typedef struct ndt_exr_params {
    int32_t pixel_type;             /* 1 half, 2 float; 0 = half */
    int32_t reserved[3];
} ndt_exr_params;
typedef struct ndt_exr_stats {
    int64_t file_bytes, raw_bytes;
    int32_t blocks, blocks_raw, launches, pad;
    double ms;
} ndt_exr_stats;
int64_t ndt_hip_exr_bound(int32_t width, int32_t rows, const ndt_exr_params *ep, int32_t with_depth);
int ndt_hip_encode_exr_device(ndt_hip_ctx *ctx, const void *d_rgba, const void *d_depth, int32_t width, int32_t rows,
                              const ndt_exr_params *ep, uint8_t *out, int64_t cap, ndt_exr_stats *stats);
int ndt_hip_encode_exr(ndt_hip_ctx *ctx, const double *rgba, const double *depth, int32_t width, int32_t rows, const ndt_exr_params *ep,
                       uint8_t *out, int64_t cap, ndt_exr_stats *stats);
int ndt_hip_render_exr(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_exr_params *ep, int32_t with_depth, uint8_t *out,
                       int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_render_ssaa_exr(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, const ndt_exr_params *ep, int32_t with_depth,
                            uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats);

/* What a pixel shows (`ndt_hip --exr --exr-aov`): the closest hit of every pixel's primary ray -- which object, where in all N
 * coordinates, and which way the surface faces there -- as planes in pixel order, and as extra channels of the frame's OpenEXR file.
 * The primary ray is the one a deterministic frame (samples == 1, no recursive_aa) starts from the pixel, the ray whose hit the depth
 * map records: row shards, NDT_STEREO_SIDE_SIDE / OVER_UNDER with the eye of the pixel's half, every camera type.  Its hit is what
 * ndt_hip_trace_rays answers for that ray with dist_limit -1, made by the same kernels; a hit within EPSILON of the ray's origin
 * counts as none (ndt.c:376: the depth map holds 0 there too).  The planes, each rows * width elements a component, [c][rows * width]:
 *   id         int32: object index + 1, 0 where the ray hits nothing
 *   position   dims planes of doubles: the hit point; all zero where id == 0
 *   normal     dims planes of doubles: the normal there as the object's intersect() returns it; all zero where id == 0
 *   ray_o / ray_v   dims planes each: the ray's origin and unit direction, for every pixel
 * A NULL member of ndt_feature_planes is not written; at least one must be set.
 *   ndt_hip_render_features          the planes into host memory
 *   ndt_hip_render_features_device   ... into the context's device memory (id aligned to 4 bytes, the doubles to 8); returns when
 *                                    they are complete.  stats (may be NULL): rays_primary, trace_launches = 1
 *   ndt_hip_features_launches        kernel launches of the context's last feature pass (primaries, trace, hit points, gather: 4)
 *   ndt_hip_exr_features_bound       ndt_hip_exr_bound for a file with the channels of `features` (a mask of NDT_FEATURE_*) of a
 *                                    dims-dimensional scene; < 0 (NDT_E_INVALID) also for dims outside 3 .. 12 and a mask that is 0
 *                                    or has unknown bits
 *   ndt_hip_encode_exr_features_device   ndt_hip_encode_exr_device with the planes d_planes names (device memory; those of the
 *                                    mask must be set) as channels.  The file's channel list, in the byte-wise order the format
 *                                    wants: A B G, N.00 .. N.<dims-1> (normal), P.00 .. P.<dims-1> (position), R, Z (with a map),
 *                                    id.  N.* and P.* are FLOAT, (float) of the doubles; id is UINT, the plane's 32 bits as they
 *                                    are; A B G R follow ndt_exr_params.  Only the groups of the mask appear.  UINT samples go
 *                                    through the two byte planes and the predictor like FLOAT ones.  4 kernel launches
 *   ndt_hip_render_exr_features      ndt_hip_render_exr, then the feature pass on the same stream, then that encoder.  The colour
 *                                    and Z channels hold the bits of the file without features
 *   ndt_hip_render_ssaa_exr_features ... for the supersampled frame: the features are the plain W x H frame's, as Z is
 * NDT_E_UNSUPPORTED with the cause in the error text, before any device work and with nothing written: recursive_aa (the pixel is
 * an average of corner samples), samples > 1 (no single primary ray), NDT_STEREO_ANAGLYPH (two rays a pixel), NDT_STEREO_HIDEF.
 * NDT_E_INVALID and NDT_E_NOMEM as the EXR entries define them: a `cap` below the file gives NDT_E_NOMEM, the size needed in the
 * error text and in stats->file_bytes, and nothing written.  Device buffers belong to the context, only grow and are reused.
 * None falls back. */
enum { NDT_FEATURE_ID = 1, NDT_FEATURE_POSITION = 2, NDT_FEATURE_NORMAL = 4 };
typedef struct ndt_feature_planes {
    int32_t *id;
    double *position, *normal, *ray_o, *ray_v;
} ndt_feature_planes;
int ndt_hip_render_features(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_feature_planes *planes, ndt_render_stats *stats);
int ndt_hip_render_features_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_feature_planes *d_planes,
                                   ndt_render_stats *stats);
int ndt_hip_features_launches(ndt_hip_ctx *ctx);
int64_t ndt_hip_exr_features_bound(int32_t width, int32_t rows, const ndt_exr_params *ep, int32_t with_depth, int32_t dims,
                                   int32_t features);
int ndt_hip_encode_exr_features_device(ndt_hip_ctx *ctx, const void *d_rgba, const void *d_depth, const ndt_feature_planes *d_planes,
                                       int32_t dims, int32_t features, int32_t width, int32_t rows, const ndt_exr_params *ep,
                                       uint8_t *out, int64_t cap, ndt_exr_stats *stats);
int ndt_hip_render_exr_features(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_exr_params *ep, int32_t with_depth,
                                int32_t features, uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_render_ssaa_exr_features(ndt_hip_ctx *ctx, const ndt_render_params *p, int32_t K, const ndt_exr_params *ep,
                                     int32_t with_depth, int32_t features, uint8_t *out, int64_t cap, ndt_exr_stats *stats,
                                     ndt_render_stats *render_stats);

/* A sampled frame denoised on the device (`ndt_hip --denoise`): an edge-avoiding a-trous wavelet over the double framebuffer, in
 * linear light, before pixel_d2c, guided by the planes of ndt_hip_render_features -- one stage between the render and the sink, as
 * supersampling is.  Defined to the bit.  Inputs: rgba = [rows][width][4] doubles; id = [rows * width] int32; position, normal =
 * [dims][rows * width] doubles.  Iteration it = 0 .. iterations - 1 has step s = 1 << it, sc = sigma_colour / (double)(1 << it),
 * inv_c = 1.0 / (sc * sc), inv_p = 1.0 / (sigma_plane * sigma_plane) (host doubles), and reads image `cur`, writes `next`.  For pixel
 * p = (y, x) with me = id[p]: me == 0 copies cur[p] bit for bit.  Otherwise num[4] = 0, den = 0, and the 25 taps are visited j outer,
 * i inner (j, i = 0 .. 4): q = (y + (j - 2) s, x + (i - 2) s), h = H[j] * H[i], H = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *   the centre tap (j == 2 and i == 2): w = h, always taken
 *   any other tap is skipped when q lies outside the image (no wrap, no clamp) or id[q] != me; otherwise, every sum over the
 *   components k = 0 .. dims - 1 in ascending order, one operation at a time:
 *       d_k = position[k][q] - position[k][p];  dd = sum d_k * d_k;  nd = sum normal[k][p] * d_k;
 *       dot = sum normal[k][p] * normal[k][q];  wn = dot > 0 ? dot : 0, then squared normal_power_log2 times
 *       wp = dd > 0 ? 1.0 - ((nd * nd) / dd) * inv_p : 1.0     (the squared sine of the angle by which q leaves p's tangent
 *                                                               hyperplane over sigma_plane^2: scale-free, no exp)
 *       cc = (q.r - p.r)^2 + (q.g - p.g)^2 + (q.b - p.b)^2 on `cur`, left to right;  wc = 1.0 / (1.0 + cc * inv_c)
 *       w = ((h * wn) * wp) * wc, and the tap is skipped unless w > 0 (which drops a NaN too)
 *   a taken tap: num[c] = num[c] + w * cur[q][c] for the four channels, then den = den + w;   finally next[p][c] = num[c] / den.
 * Only + - * / and comparisons on doubles, none contracted: a restatement in plain C or numpy gives the same 64-bit patterns.
 *   ndt_hip_denoise_device           the filter alone on the context's device memory: d_rgba_in and d_rgba_out rows x width x 4
 *                                    doubles aligned to 16 bytes (they may be the same), the id, position and normal members of
 *                                    d_planes set and aligned to their elements.  One launch an iteration; synchronous; no scene needed
 *   ndt_hip_render_denoised_device   on the context's one stream: the frame `p` asks for, any samples, through ndt_hip_render_device;
 *                                    the feature pass of a copy of `p` whose samples is 1 -- the guide of a pixel is the hit of
 *                                    the ray a deterministic frame starts from it; then the iterations into d_rgba (aligned to 16)
 *   ndt_hip_render_denoised          the same into host memory
 *   ndt_hip_render_denoised_rgba8 / _png / _jpeg / _exr   the same doubles through ndt_hip_quantize_device and the encoders of
 *                                    the 8-bit files, or through ndt_hip_encode_exr_device (colour only)
 *   ndt_hip_denoise_launches / ndt_hip_denoise_ms   kernel launches of the context's last call (4 + iterations after a rendered
 *                                    frame, iterations after ndt_hip_denoise_device), and the iterations' summed device time
 * dp == NULL: the defaults (a first guess from a synthetic frame).  NDT_E_UNSUPPORTED with the cause in the error text, before any
 * device work and with nothing written: recursive_aa; any stereo mode but mono (a stencil must not cross the seam between two
 * eyes); row_begin != 0 or row_step != 1 (a cyclic shard has no neighbouring rows).  NDT_E_INVALID: parameters out of range, a NaN
 * sigma, NULL or misaligned pointers or planes, dims outside 3 .. 12.  The device buffers belong to the context, only grow and are
 * reused.  None falls back. */
typedef struct ndt_denoise_params {
    int32_t iterations;             /* 1 .. 6; default 4 */
    int32_t normal_power_log2;      /* 0 .. 8; default 5: the normals' dot product to the power 32 */
    double  sigma_colour;           /* finite, > 0; default 0.25 */
    double  sigma_plane;            /* finite, > 0; default 0.25 */
} ndt_denoise_params;
int ndt_hip_denoise_device(ndt_hip_ctx *ctx, const void *d_rgba_in, const ndt_feature_planes *d_planes, int32_t dims, int32_t width,
                           int32_t rows, const ndt_denoise_params *dp, void *d_rgba_out);
int ndt_hip_render_denoised_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, void *d_rgba,
                                   ndt_render_stats *stats);
int ndt_hip_render_denoised(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, double *rgba,
                            ndt_render_stats *stats);
int ndt_hip_render_denoised_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, uint8_t *rgba8,
                                  ndt_render_stats *stats);
int ndt_hip_render_denoised_png(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, uint8_t *png, int64_t cap,
                                ndt_png_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_render_denoised_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, const ndt_jpeg_params *jp,
                                 uint8_t *jpg, int64_t cap, ndt_jpeg_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_render_denoised_exr(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, const ndt_exr_params *ep,
                                uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_denoise_launches(ndt_hip_ctx *ctx);
double ndt_hip_denoise_ms(ndt_hip_ctx *ctx);

/* The sample moments of a frame: beside the frame, what the adaptive loop of the stochastic paths (samples > 1, area lights)
 * consumed for every pixel -- the input of the variance-guided denoiser below.
 *   rgba    what ndt_hip_render_device gives for `p`, bit for bit
 *   count   [rows * width] int32: the samples the loop consumed for the pixel
 *   sum_sq  [3][rows * width] doubles: for c = r, g, b, 0.0 and then sum_sq_c = sum_sq_c + l_c * l_c for the colour l of each
 *           consumed sample, in the order consumed
 * A frame that does not go through the loop (samples == 1 on a scene without area lights) has count = 1 and sum_sq_c = rgba_c *
 * rgba_c, from one small launch.  Option "sample_cap" bounds count.  NDT_E_UNSUPPORTED with the cause in the error text, before any
 * device work and with nothing written: recursive_aa, NDT_STEREO_ANAGLYPH, NDT_STEREO_HIDEF.  Row shards and NDT_STEREO_SIDE_SIDE /
 * OVER_UNDER work.  _device: device memory (count aligned to 4 bytes, sum_sq to 8); the other: host memory.  Synchronous. */
int ndt_hip_render_moments_device(ndt_hip_ctx *ctx, const ndt_render_params *p, void *d_rgba, void *d_count, void *d_sum_sq,
                                  ndt_render_stats *stats);
int ndt_hip_render_moments(ndt_hip_ctx *ctx, const ndt_render_params *p, double *rgba, int32_t *count, double *sum_sq,
                           ndt_render_stats *stats);

/* The variance of every pixel's mean, summed over r, g, b, from the moments (kernel k_sample_variance: one lane a pixel, one launch;
 * device memory; synchronous).  Defined to the bit, for n = count[p]: n < 2 gives 0.0.  Otherwise v = 0 and, for c = r, g, b in
 * turn:  m = rgba[p][c];  e = sum_sq[c][p] / (double)n - m * m;  e = e > 0 ? e : 0.0;  v = v + e / (double)(n - 1).
 * variance[p] = v, [rows * width] doubles: in the units of the filter's squared colour distance. */
int ndt_hip_sample_variance_device(ndt_hip_ctx *ctx, const void *d_rgba, const void *d_count, const void *d_sum_sq, int32_t width,
                                   int32_t rows, void *d_variance);

/* The variance-guided denoiser (`ndt_hip --vdenoise`): the a-trous filter above with the width of its colour weight taken from the
 * frame, pixel by pixel, and the variance carried through the iterations.  It filters where the frame is noisy; where it has
 * converged it copies the pixel bit for bit.  Defined to the bit.  Inputs: those of ndt_hip_denoise_device, and variance =
 * [rows * width] doubles.  Iteration it = 0 .. iterations - 1 has step s = 1 << it, reads (cur, vcur) and writes (next, vnext);
 * k2 = k_colour * k_colour and inv_p = 1.0 / (sigma_plane * sigma_plane) are host doubles.  For pixel p = (y, x) with me = id[p]:
 *   me == 0: next[p] and vnext[p] are cur[p] and vcur[p], bit for bit.
 *   the local variance, at distance 1 whatever the step: gn = 0, gd = 0; r = (y + b - 1, x + a - 1) for b outer, a inner over
 *       0 .. 2, g = G[b] * G[a], G = {1/4, 1/2, 1/4}; r is skipped when it lies outside the image or id[r] != me, otherwise
 *       gn = gn + g * vcur[r];  gd = gd + g.   sp = k2 * (gn / gd).
 *   !(sp > 0) -- zero, negative or a NaN: next[p] and vnext[p] are copied bit for bit: the pixel has converged.
 *   otherwise the 25 taps of the definition above in the same order: h, wn, wp as there, cc on `cur`, and
 *       wc = 1.0 / (1.0 + cc / sp);  w = ((h * wn) * wp) * wc, the tap skipped unless w > 0; the centre always taken with w = h.
 *       a taken tap, the centre too: num[c] = num[c] + w * cur[q][c] for the four channels, then den = den + w, then
 *       vn = vn + (w * w) * vcur[q].   Finally next[p][c] = num[c] / den and vnext[p] = vn / (den * den).
 * Only + - * / and comparisons on doubles, none contracted.
 *   ndt_hip_vdenoise_device          the filter alone on the context's device memory: arguments, alignments and the in-place rule of
 *                                    ndt_hip_denoise_device; d_variance and d_variance_out aligned to 8 bytes, d_variance_out may be
 *                                    NULL (the last plane is dropped) or d_variance.  One launch an iteration; synchronous
 *   ndt_hip_render_vdenoised_device  on the context's one stream: ndt_hip_render_moments_device for `p`; the feature pass of a copy of
 *                                    `p` whose samples is 1; k_sample_variance; the iterations into d_rgba (aligned to 16)
 *   ndt_hip_render_vdenoised         the same into host memory;  _rgba8 / _png / _jpeg / _exr: as ndt_hip_render_denoised's
 * ndt_hip_denoise_launches / ndt_hip_denoise_ms report the context's last call of either filter: 4 + 1 + iterations launches after
 * a frame rendered here, iterations after ndt_hip_vdenoise_device.  vp == NULL: the defaults.  Refusals: those of the denoiser
 * above, and what the moments refuse.  None falls back. */
typedef struct ndt_vdenoise_params {
    int32_t iterations;             /* 1 .. 6; default 4 */
    int32_t normal_power_log2;      /* 0 .. 8; default 5 */
    double  k_colour;               /* finite, > 0; default 4.0: the colour weight halves at k_colour local standard deviations */
    double  sigma_plane;            /* finite, > 0; default 0.25 */
} ndt_vdenoise_params;
int ndt_hip_vdenoise_device(ndt_hip_ctx *ctx, const void *d_rgba_in, const ndt_feature_planes *d_planes, const void *d_variance,
                            int32_t dims, int32_t width, int32_t rows, const ndt_vdenoise_params *vp, void *d_rgba_out,
                            void *d_variance_out);
int ndt_hip_render_vdenoised_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, void *d_rgba,
                                    ndt_render_stats *stats);
int ndt_hip_render_vdenoised(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, double *rgba,
                             ndt_render_stats *stats);
int ndt_hip_render_vdenoised_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, uint8_t *rgba8,
                                   ndt_render_stats *stats);
int ndt_hip_render_vdenoised_png(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, uint8_t *png, int64_t cap,
                                 ndt_png_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_render_vdenoised_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, const ndt_jpeg_params *jp,
                                  uint8_t *jpg, int64_t cap, ndt_jpeg_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_render_vdenoised_exr(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, const ndt_exr_params *ep,
                                 uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats);

/* Ambient occlusion of a frame on the device (`ndt_hip --ao`): how open the surface a pixel shows is to its surroundings, in all N
 * coordinates -- geometry only, from the planes of ndt_hip_render_features.  One stage between the render and the sink, as the
 * denoiser is.  Inputs, of the rows `p` selects: id = [rows * width] int32; position, normal, ray_v = [dims][rows * width] doubles, the
 * feature planes of the deterministic frame (samples == 1).  Output: ao = [rows * width] doubles in 0 .. 1, 1.0 = open.
 * For pixel p = (row j of the image, column i) with id[p] != 0, every sum over the components k = 0 .. dims - 1 in ascending order,
 * one operation at a time, starting from 0.0:
 *     len = sqrt(sum normal[k][p]^2).  !(len > 0) or len not finite: ao[p] = 1.0, and the pixel sends no rays.
 *     n'_k = normal[k][p] / len, every component negated when sum n'_k * ray_v[k][p] > 0: the hemisphere faces the viewer.
 *     origin = position[.][p] itself, as a reflection ray's is (ndt.c:398-402); the intersectors reject t <= EPSILON themselves.
 * Sample s = 0 .. samples - 1 has its own counter-based stream (ndt_device.hpp: ndt_rng_mix is splitmix64's finaliser):
 *     key = ndt_rng_mix(ndt_rng_mix((j * width + i) * 0x100000001b3 + s) ^ 0x616f2d72617973 ^ ndt_rng_mix(seed)),
 *     u_m = ndt_rng_uniform(key, m) = (ndt_rng_mix(key + m) >> 11) * 2^-53,   m = 0 .. 2 * ceil(dims / 2) - 1
 * -- of the image pixel, not the shard's; independent of sharding, of batching and of `samples`: sample s of a call is sample s of
 * every call with more; the constant keeps the streams apart from those of samples > 1.  The direction is uniform over the hemisphere:
 *     pair m: r = sqrt(-2.0 * log(1.0 - u_2m)), a = (2.0 * M_PI) * u_2m+1, g_2m = r * cos(a), g_2m+1 = r * sin(a)  (Box-Muller; the
 *     last of an odd dims is not used);   d_k = g_k / sqrt(sum g_k^2);   c = sum d_k * n'_k;   c < 0: d = -d, c = -c.
 * log, cos and sin are the device's, so a restatement elsewhere need not give their last bits: every entry can return the directions
 * it used ([samples][dims][rows * width] doubles, zero where the pixel sends no rays), and everything behind them is defined to the bit:
 *     radius == 0: the ray (origin, d) is occluded <=> ndt_hip_trace_rays answers an object >= 0 for it with dist_limit 0
 *     radius > 0:  ... <=> its closest hit (dist_limit -1) exists and v_dist(hit, origin) < radius, v_dist = the root of (the even
 *                  components' sum of squared differences + the odd ones') as vectNd_dot sums (vectNd.h:215-227)
 *     den = sum_s c_s;  num = sum_s (occluded_s ? 0 : c_s), both over s ascending;   ao[p] = den > 0 ? num / den : 1.0
 * and ao[p] = 1.0 where id[p] == 0.  The cosine-weighted share of the hemisphere that is open.
 *   ndt_hip_ao_device            the pass alone: d_planes' id, position, normal and ray_v (device memory, aligned to their elements)
 *                                of the rows `p` selects of the uploaded scene, into d_ao and, unless NULL, d_dirs (device, 8 bytes).
 *                                Per batch of samples 3 kernel launches (rays, trace, fold), 4 with a radius (hit points); synchronous
 *   ndt_hip_render_ao_device     the feature pass of a copy of `p` whose samples is 1, then that pass
 *   ndt_hip_render_ao            the same into host memory (dirs may be NULL)
 *   ndt_hip_ao_apply_device      out.rgb = in.rgb * ((1.0 - strength) + strength * ao), alpha copied; rows x width x 4 doubles aligned
 *                                to 16 bytes, out may be in.  strength 0 leaves the image bit for bit.  One launch; no scene needed
 *   ndt_hip_render_ao_shaded_device   ndt_hip_render_device for `p` as given (any samples), the pass of its deterministic twin, the
 *                                apply with ap->strength, into d_rgba (16 bytes); d_ao, unless NULL, receives the plane
 *   ndt_hip_render_ao_shaded     the same into host memory (ao may be NULL);  _rgba8 / _png / _jpeg: the same doubles through
 *                                ndt_hip_quantize_device and the encoders of the 8-bit files
 *   ndt_hip_exr_ao_bound         ndt_hip_exr_features_bound for a file that also carries the channel AO; the mask may be 0
 *   ndt_hip_encode_exr_ao_device ndt_hip_encode_exr_features_device with the FLOAT channel AO, (float) of the plane d_ao: the channel
 *                                list in the format's byte-wise order is A AO B G N.* P.* R Z id.  The mask may be 0
 *   ndt_hip_render_exr_ao        ndt_hip_render_depth_device, the pass, the colour multiplied as by the apply (strength 0: the colour,
 *                                Z and feature channels hold the bits of the file without AO), the feature planes, that encoder
 *   ndt_hip_ao_launches / ndt_hip_ao_ms   kernel launches of the context's last call (the feature pass's 4 and the apply's 1 included
 *                                where they run), and the device time of its pass
 * Option "ao_batch" (ndt_hip_set_option) sets how many samples share a trace launch; the plane does not depend on it.
 * ap == NULL: the defaults (a first guess, not measured against anything).  NDT_E_UNSUPPORTED with the cause in the error text, before
 * any device work and with nothing written: recursive_aa, NDT_STEREO_ANAGLYPH, NDT_STEREO_HIDEF; samples > 1 for ndt_hip_ao_device,
 * whose planes are one deterministic frame's (every other entry makes them itself).  NDT_E_INVALID: parameters out of range, a NaN, NULL or misaligned
 * pointers, dims outside 3 .. 12.  NDT_E_STATE: no scene.  Row shards and NDT_STEREO_SIDE_SIDE / OVER_UNDER work: a pixel needs no
 * neighbour.  The device buffers belong to the context, only grow and are reused.  None falls back. */
typedef struct ndt_ao_params {
    int32_t  samples;               /* 1 .. 256; default 16 */
    int32_t  reserved;              /* must be 0 */
    double   radius;                /* finite, >= 0; 0 (default): no limit, any hit occludes */
    uint64_t seed;                  /* default 0 */
    double   strength;              /* 0 .. 1; default 1 */
} ndt_ao_params;
int ndt_hip_ao_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_feature_planes *d_planes, const ndt_ao_params *ap, void *d_ao,
                      void *d_dirs);
int ndt_hip_render_ao_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, void *d_ao, void *d_dirs,
                             ndt_render_stats *stats);
int ndt_hip_render_ao(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, double *ao, double *dirs,
                      ndt_render_stats *stats);
int ndt_hip_ao_apply_device(ndt_hip_ctx *ctx, const void *d_rgba_in, const void *d_ao, int64_t n_pixels, double strength, void *d_rgba_out);
int ndt_hip_render_ao_shaded_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, void *d_rgba, void *d_ao,
                                    ndt_render_stats *stats);
int ndt_hip_render_ao_shaded(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, double *rgba, double *ao,
                             ndt_render_stats *stats);
int ndt_hip_render_ao_shaded_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, uint8_t *rgba8,
                                   ndt_render_stats *stats);
int ndt_hip_render_ao_shaded_png(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, uint8_t *png, int64_t cap,
                                 ndt_png_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_render_ao_shaded_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_ao_params *ap, const ndt_jpeg_params *jp,
                                  uint8_t *jpg, int64_t cap, ndt_jpeg_stats *stats, ndt_render_stats *render_stats);
int64_t ndt_hip_exr_ao_bound(int32_t width, int32_t rows, const ndt_exr_params *ep, int32_t with_depth, int32_t dims, int32_t features);
int ndt_hip_encode_exr_ao_device(ndt_hip_ctx *ctx, const void *d_rgba, const void *d_depth, const ndt_feature_planes *d_planes,
                                 const void *d_ao, int32_t dims, int32_t features, int32_t width, int32_t rows, const ndt_exr_params *ep,
                                 uint8_t *out, int64_t cap, ndt_exr_stats *stats);
int ndt_hip_render_exr_ao(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_exr_params *ep, int32_t with_depth, int32_t features,
                          const ndt_ao_params *ap, uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats);
int ndt_hip_ao_launches(ndt_hip_ctx *ctx);
double ndt_hip_ao_ms(ndt_hip_ctx *ctx);

/* ONE frame over several contexts -- one per GPU of the node, or several on one GPU -- called from one host thread.
 * The rows `p` selects are dealt cyclically to the contexts exactly as the reference deals rows to MPI ranks in
 * MPI_MODE_ROW (ndt.c:812-820: row_start = rank, row_step = size): context k renders rows
 * p->row_begin + (k + i*n_ctx)*p->row_step.  Every context must hold the same uploaded scene.  Each device pushes
 * its finished rows straight into the assembled image on ctxs[0]'s device (peer stores over xGMI; through a staging
 * copy where peer access is unavailable or option "multi_path" asks for it) -- the reference instead sum-reduces full-size zero-padded images up a
 * binary tree (mpi_collect_image, ndt.c:1277-1309).  `format` = ndt_image_format.  _device: `d_out` is memory of
 * ctxs[0]'s device; plain: `out` is host memory.  stats: ray counts summed over the contexts, times = the slowest's.
 * Not with a depth map.  Returns when the image is complete. */
int ndt_hip_render_multi_device(ndt_hip_ctx *const *ctxs, int32_t n_ctx, const ndt_render_params *p, int32_t format,
                                void *d_out, ndt_render_stats *stats);
int ndt_hip_render_multi(ndt_hip_ctx *const *ctxs, int32_t n_ctx, const ndt_render_params *p, int32_t format,
                         void *out, ndt_render_stats *stats);

/* How a context's rows reached the assembled image in the last ndt_hip_render_multi[_device] call it took part in, so
 * that a multi-GPU run can be diagnosed from its log (option "multi_path" chooses; `ndt_hip -g N` prints it):
 * LOCAL = the context lives on ctxs[0]'s device; PEER = its push kernel stored over xGMI into ctxs[0]'s HBM;
 * STAGED = one hipMemcpyPeerAsync into a staging buffer on ctxs[0]'s device, pushed from there; NONE = no rows. */
enum ndt_multi_path { NDT_MULTI_NONE = 0, NDT_MULTI_LOCAL = 1, NDT_MULTI_PEER = 2, NDT_MULTI_STAGED = 3 };
int ndt_hip_multi_path_taken(ndt_hip_ctx *ctx);

/* Switches of a context.  None but "sample_seed" and "sample_cap" changes an image; they choose between equivalent ways of
 * producing it, or turn diagnostics on.  The same names, upper-cased behind NDT_HIP_ (NDT_HIP_PIPELINE, NDT_HIP_DEBUG_LEVELS ...), are read from the
 * environment ONCE, when the context is created; nothing on the render or upload path looks at the environment.
 *   "pipeline"        0 auto, 1 levels (one trace launch + shade launches per bounce), 2 stream (the whole ray tree in
 *                     one persistent launch) -- DESIGN.md section 3; the environment takes the words
 *   "stream_below"    auto: passes of up to this many primaries go to the streaming frame kernel
 *   "stream_below_list"  ... and passes over a list of samples (recursive anti-aliasing) of up to this many (default 30 000)
 *   "hull_box" / "face_box"   0: upload hcubes without the hull box / without the per-face boxes (tests prove them neutral)
 *   "face_tree"               0: hcubes of more than 63 faces without the hierarchy over their face boxes (ndt_hip_hcube_face_tree;
 *                                tests prove it neutral)
 *   "face_groups"             0: ... without the index of their faces by thin hull axes (ndt_hip_hcube_face_groups; neutral)
 *   "fuse_primaries"          per-bounce kernels: -1 auto (the first trace launch makes the primaries itself for a planar
 *                                camera from 4-D on), 0 always a k_primary launch, 1 never one (planar camera)
 *   "gate_prepass_below"      item-set scenes: passes of up to this many primaries mark the items whose bounding sphere the
 *                                ray's line misses as visited before the walk (neutral; default 400 000)
 *   "stream_fused"            0: the frame kernel between a k_primary and a k_finish_pixels launch instead of making its
 *                                primaries and writing its pixels itself (tests prove it neutral)
 *   "item_sets"               0: upload a scene of up to 64 items with plain leaf lists (the kernels that read the lists,
 *                                as for larger scenes) instead of 64-bit item sets per leaf (tests prove it neutral)
 *   "item_boxes"              0: upload scenes of more than 256 items without the item boxes (ndt_hip_item_boxes)
 *   "leaf_scan" / "leaf_scan_group"   global-memory tier: the lanes of a wavefront that stand on the same kd leaf scan it
 *                                together through LDS (0: never) when at least that many of them do (default 64: all)
 *   "leaf_history"            scenes in the global-memory tier (more than 256 items): a ray remembers what it visited as up to
 *                                this many {leaf, cut} pairs (default and maximum 4) before it falls back to its bit mask in
 *                                the slab; 0: the slab only (tests prove every value neutral)
 *   "sample_seed"     stochastic renders (-n > 1, area lights): which set of counter-based random streams the samples draw
 *                     from (0, the default, and any other value give images that are independent draws of one distribution)
 *   "sample_cap"      stochastic renders: 0 (default) no cap -- `samples` is a lower bound, a pixel goes on sampling while its running
 *                     mean moves by more than 1/256; C >= 1: no pixel takes more than C samples and no pass renders past them
 *                     (C <= samples: exactly C a pixel, one pass, aa_samples = C x pixels).  It names no stream: sample r of a pixel
 *                     is the same sample with and without a cap.  Wherever the loop runs: samples > 1, area lights, the list renders
 *                     of recursive_aa, both eyes of an anaglyph.  A negative value: NDT_E_INVALID
 *   "multi_path"      ndt_hip_render_multi: 0 auto (stores on the same device, peer stores over xGMI, a staged copy where
 *                     there is no peer access), 1 never staged, 2 always staged -- also between contexts of one device
 *   "light_overlap"   per-bounce pipeline, one light window: 1 (default) the lighting of every bounce but the deepest runs
 *                     on the context's second stream beside the next bounce's trace launch; 0 every launch on the one stream,
 *                     the lighting of a bounce in front of the shading of the next.  Same image, same counts
 *   "early_pixels"    where "light_overlap" applies (a no-op elsewhere): the pixels of primaries that are final long before the
 *                     end of the frame are finished on the second stream, and the frame's last launch takes the rest.  0 off;
 *                     1 (default) the primaries that hit nothing, beside the second trace launch; 2 also the hit ones without
 *                     a reflection or refraction ray, behind the lighting of the primaries.  Same image, same counts
 *   "light_window"    lights the lighting kernels take per window: 0 (default) auto, windows of 64; k in 1..64 at most k
 *                     list entries a window (ambient ones included).  A scene of more than one window renders every pass
 *                     with the per-bounce kernels, whatever "pipeline" says, and pays a shading and a trace launch per
 *                     bounce and extra window.  Neutral: it exists so that tests can run the window path on any scene
 *   "ao_batch"        ambient occlusion (ndt_hip_render_ao*): samples that share one trace launch.  0 (default) auto: as many as fit
 *                     2^23 workspace slots, at least one; n in 1 .. 256: exactly n (the last launch takes what is left).  Same plane
 *   "debug_levels"    profiled renders print the bounces and the duration of every trace launch
 *   "exit_probe" / "shade_probe" / "stream_probe"   profiled renders log the life of every wavefront of the trace
 *                     launches / of the k-th shade launch (value k + 1) / of the frame kernel
 *   "test_small_pool" a fresh workspace starts with a node pool a reflective scene overflows (tests of the regrow path)
 * Returns NDT_E_INVALID for a name it does not know. */
int ndt_hip_set_option(ndt_hip_ctx *ctx, const char *name, int64_t value);

/* HIP devices this process sees (0 without a GPU), and the device a context lives on. */
int ndt_hip_device_count(void);
int ndt_hip_device(ndt_hip_ctx *ctx);

/* Number of rows a (row_begin,row_step) shard of a `height`-row image holds. */
int32_t ndt_hip_shard_rows(int32_t height, int32_t row_begin, int32_t row_step);

/* Diagnostic, host only (no GPU needed): the hull box the library derives for hcube `object`
 * of `scene` at upload time -- an oriented box that contains every point orthotope.intersect
 * (orthotope.c:150-300) can return for the hcube's faces; rays that miss it skip the nested
 * trace() over the faces (hcube.c:241), which cannot change the answer.  rows receives
 * dims x { unit axis[dims], centre coordinate, half extent }: the region |axis_k . x - centre_k| <= half_k for every k.  The
 * axes are unit covectors -- an orthonormal frame, or, when the hcube is a parallelotope, the normalised dual basis of its
 * edge directions (axis_k . d_j = 0 for j != k), in which every face is thin exactly on the directions it does not span;
 * they need not be orthogonal to each other.  Returns 1 when the hcube has a
 * box, 0 when it has none (its faces are always scanned), <0 on NDT_E_*. */
int ndt_hip_hcube_hull_box(const ndt_flat_scene *scene, int32_t object, double *rows);

/* Diagnostic, host only: the boxes of the single faces of hcube `object` in the frame of its hull box
 * (same derivation, one face at a time): the nested trace() visits only the faces whose box the ray
 * meets.  face_rows receives n_faces x dims x { centre coordinate, half extent } (room for 63 faces);
 * bit f of *possible is clear when face f can never be hit.  Returns the number of faces, 0 when the
 * hcube has no hull box, or more than 63 faces (then: ndt_hip_hcube_face_boxes_all), <0 on NDT_E_*. */
int ndt_hip_hcube_face_boxes(const ndt_flat_scene *scene, int32_t object, double *face_rows, uint64_t *possible);
/* ... for an hcube of any number of faces (a 6-D one nests 472, a 10-D one 52 904: the device takes their boxes 63 at a time):
 * face_rows: n_faces x dims x { centre, half extent }, possible: one byte per face.  Returns the number of faces; with
 * cap_faces too small (or null pointers) only that -- call again with room.  0: the hcube gets no boxes, <0 on NDT_E_*. */
int64_t ndt_hip_hcube_face_boxes_all(const ndt_flat_scene *scene, int32_t object, int64_t cap_faces, double *face_rows, uint8_t *possible);
/* Diagnostic, host only: the hierarchy the library lays over the face boxes of an hcube of more than 63 faces (option
 * "face_tree"): level j = 1 .. *top holds, for every aligned run [k 2^j, (k + 1) 2^j) of faces, the box of the union of the
 * boxes of its faces that can be hit (half extents of -1: none can); a ray that misses a run's box skips its faces.
 * rows: n_nodes x dims x { centre, half extent }, level j starting at node level_off[j] (level_off: room for 32 ints).
 * Returns the number of nodes; with cap_nodes too small (or rows null) only that and *top.  0: no boxes, <0 on NDT_E_*. */
int64_t ndt_hip_hcube_face_tree(const ndt_flat_scene *scene, int32_t object, int64_t cap_nodes, double *rows, int32_t *level_off, int32_t *top);

/* Diagnostic, host only: the index the library lays over the faces of an hcube of more than 63 faces in 5-D and up (option
 * "face_groups"): the faces by the set of hull axes their boxes are thin on.  clusters: dims x { centre-, half-, centre+, half+ }
 * -- per hull axis the two intervals (one per side of the hull's centre; half -1: none) that hold the thin intervals of all
 * faces thin on that axis; table: 2^dims x { start, count } -- for every subset S of the axes where in `members` (n_faces
 * ints, may be null) the faces thin exactly on S stand, ascending; face_set: per face its S as a bit mask (-1: the face can
 * never be hit).
 * A ray can meet a face's box only if, inside the hull box, it passes a cluster interval on every axis of the face's S; the
 * device looks up the subsets of the axes whose clusters the ray passes and tests their faces' own boxes.
 * Returns the number of faces (0: the hcube gets no boxes), <0 on NDT_E_*. */
int ndt_hip_hcube_face_groups(const ndt_flat_scene *scene, int32_t object, double *clusters, int32_t *table, int32_t *face_set, int32_t *members);

/* Diagnostic, host only: the item boxes the library derives at upload for scenes of more than 256 items -- one orthonormal
 * frame for the scene (frame: dims x unit axis[dims]) and, for every top-level orthotope, the box in that frame of every
 * point its intersect() can return (rows: n_items x dims x { centre coordinate, half extent }; has[i] != 0: item i carries
 * one).  A ray that misses an item's box skips its bounding-sphere gate and its intersect(); tests prove that neutral.
 * Returns the number of boxed items (0: none), <0 on NDT_E_*. */
int ndt_hip_item_boxes(const ndt_flat_scene *scene, double *frame, double *rows, uint8_t *has);

/* What upload accepts.  Host only (no GPU, no context): NDT_OK, or the code ndt_hip_upload_scene would refuse `scene` with and
 * its message in ndt_hip_last_error().  ndt_hip_upload_scene calls this first and builds nothing for a scene it refuses; a
 * refused upload (or one that fails later, on the device) leaves the context WITHOUT a scene -- the one it held is gone, every
 * render answers NDT_E_STATE until an upload succeeds -- and nothing of the refused scene stays behind in it.
 *
 * The rules, tried in this order; the first one broken is the answer.  NDT_E_INVALID unless marked [U] = NDT_E_UNSUPPORTED.
 * "A vector range (off, k)" is k vectors at vecs + off: off >= 0, k >= 0, off + k * dims <= n_vecs.  A message about an object,
 * a kd node or a light names it: "object 7: ...", "kd node 3: ...", "light 2: ...".
 *   1. abi_version == NDT_HIP_ABI_VERSION; [U] NDT_MIN_DIMS <= dims <= NDT_MAX_DIMS; [U] 0 <= cam_type <= 2; cam_type != 0
 *      needs cam_local_x_off, cam_local_y_off, cam_local_z_off >= 0.
 *   2. Counts: n_lights, n_objects, n_items, n_kd_nodes, n_leaf_refs, n_inf, n_vecs, n_sizes, n_flags, n_obj_refs >= 0 (the message
 *      names the count); [U] n_lights <= NDT_MAX_LIGHTS; n_items <= n_objects.  A count says how many entries of its array may be read: the library
 *      reads none beyond it and cannot know of a count larger than the memory behind the pointer.
 *   3. An array with a positive count is not NULL: vecs, sizes, flags, obj_refs, lights, objects, kd_nodes, leaf_refs, inf_refs.
 *   4. The kd-tree, when n_kd_nodes > 0, walked from node 0 (level 1), a node, then its left subtree, then its right one; nodes
 *      the walk does not reach are not read.  [U] No node stands deeper than level 40 (the traversal stack; the walk itself goes
 *      no deeper).  No node is reached twice (reported as that node).  Interior node (dim >= 0): dim < dims; left and right are
 *      node indices, 0 <= . < n_kd_nodes (reported as the node that holds the index).  Leaf (dim < 0): num >= 0, first >= 0,
 *      first + num <= n_leaf_refs, and every listed entry is an item, 0 <= . < n_items.
 *   5. Every entry of inf_refs is an item.
 *   6. Every object, in order: [U] 0 <= type < NDT_OBJ_TYPE_COUNT; (bounds_center_off, 1), (pos_off, n_pos) and (dir_off, n_dir)
 *      are vector ranges; n_size >= 0, size_off >= 0, size_off + n_size <= n_sizes; the same for n_flag, flag_off and n_flags;
 *      then what its plugin reads: sphere 1 pos, 1 size; hplane 1 pos, 1 dir; hdisk 1 pos, 1 dir, 1 size; cylinder 2 pos, 1 size;
 *      hcylinder dims - 1 pos, 1 size; orthotope 1 pos, 1 flag and 0 <= flags[flag_off] <= min(n_dir, dims); hfacet 3 pos, 1 flag,
 *      and 3 dir when flags[flag_off] != 0; facet 3 pos, 1 dir; hcube: [U] n_obj >= 1 (the faces add_faces makes, hcube.c:34),
 *      obj_off >= 0, obj_off + n_obj <= n_obj_refs, every child an object index, 0 <= . < n_objects, of an object that is no
 *      hcube.  n_obj / obj_off of other types and `parent` are not read.
 *   7. (bb_lower_off, 1) and (bb_upper_off, 1) are vector ranges.
 *   8. Every light, in order: 0 <= type <= NDT_LIGHT_RECT; DISK / RECT: (area_off, 2); POINT / SPOT / DISK / RECT: (pos_off, 1);
 *      DIRECTIONAL / SPOT: (dir_off, 1) are vector ranges.  Offsets a type does not use are not read.
 *   9. The camera: (cam_pos_off, 1), (cam_img_orig_off, 1), (cam_dir_x_off, 1), (cam_dir_y_off, 1), and each of cam_left_eye_off,
 *      cam_right_eye_off, cam_local_x_off, cam_local_y_off, cam_local_z_off that is >= 0 (negative: the scene has none).
 * A NULL `scene` is refused with NDT_E_INVALID like any other, by either entry, and costs the context its scene as well.
 * Reals are not judged.  Scenes with no light, no kd node, no infinite object, no item or no object at all pass. */
int ndt_hip_check_scene(const ndt_flat_scene *scene);

/* The stream the context launches on (a hipStream_t, created hipStreamNonBlocking: nothing the caller queues on the NULL
 * stream or any other is ordered against it implicitly), for callers that time with their own events or order other work
 * against it. */
void *ndt_hip_stream(ndt_hip_ctx *ctx);
int ndt_hip_synchronize(ndt_hip_ctx *ctx);

const char *ndt_hip_last_error(void);
int ndt_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NDT_HIP_H */
