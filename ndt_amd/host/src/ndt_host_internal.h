/* ndt_host_internal.h -- shared between the host sources; not part of the scene API. */
#ifndef NDT_HOST_INTERNAL_H
#define NDT_HOST_INTERNAL_H
#include "ndt_host_api.h"
#include "../../../include/ndt_hip.h"

#define NDT_TYPE_CLUSTER 100
#define NDT_TYPE_OTHER 101

const char *ndt_object_plugin_file(const char *type);    /* file of a host-side-only plugin type, or NULL */
int ndt_object_type_id(object *o);                  /* NDT_OBJ_* for device types, else NDT_TYPE_* */
int ndt_object_has_default_material(object *o);
void ndt_hcube_prepare(object *cube);

/* ---- kd-tree as the reference builds it (kd-tree.c:294-477) ---- */
typedef struct {
    double *lower, *upper;          /* dims each */
    int id;
    object *obj;
} ndt_kd_item;

typedef struct ndt_kd_node {
    int dim;                        /* split dimension, -1 for a leaf */
    double boundary;
    int num;                        /* leaf: number of items */
    int *ids;                       /* leaf: item ids, in list order */
    struct ndt_kd_node *left, *right;
} ndt_kd_node;

typedef struct {
    int dims;
    ndt_kd_item *items; int n_items, cap_items;
    int *inf_ids; int n_inf;
    double *bb_lower, *bb_upper;
    ndt_kd_node *root;
} ndt_kd_tree;

void ndt_kd_init(ndt_kd_tree *t, int dims);
void ndt_kd_add_object(ndt_kd_tree *t, object *obj);        /* object_kdlist_add, object.c:633-681 */
void ndt_kd_build(ndt_kd_tree *t);                          /* kd_tree_build, kd-tree.c:421-477 */
void ndt_kd_free(ndt_kd_tree *t);

/* kd_tree_build over flat arrays (ndt_kdtree.c): the CPU twin of ndt_hip_build_kdtree, the specification the device build is
 * compared with.  The arrays are malloc'ed: whoever takes the tree frees them with free() or ndt_host_kdtree_free.
 * Returns 0, or -1 for arguments the device call refuses as well. */
typedef struct {
    int32_t n_kd_nodes, n_leaf_refs, n_inf;
    int32_t depth;                  /* levels: 1 for a single leaf */
    ndt_flat_kdnode *nodes;         /* preorder */
    int32_t *leaf_refs, *inf_refs;
    double *bb_lower, *bb_upper;    /* dims each */
} ndt_host_kdtree;
int ndt_host_build_kdtree(int dims, int n_items, const double *lower, const double *upper, const unsigned char *finite, ndt_host_kdtree *out);
void ndt_host_kdtree_free(ndt_host_kdtree *t);

/* ---- flattening (the reference-side stub of INTEGRATION.md, against this host model) ---- */
typedef struct {
    ndt_flat_scene fs;
    double *vecs;   long n_vecs, cap_vecs;
    double *sizes;  long n_sizes, cap_sizes;
    int *flags;     long n_flags, cap_flags;
    int *refs;      long n_refs, cap_refs;
    ndt_flat_object *objects; int n_objects, cap_objects;
    ndt_flat_light *lights;   int n_lights;
    ndt_flat_kdnode *nodes;   int n_nodes, cap_nodes;
    int *leaf_refs; int n_leaf_refs, cap_leaf_refs;
    int *inf_refs;  int n_inf;
} ndt_flat_builder;

/* Builds bounds + kd-tree exactly like ndt.c:1899-1908, aims the camera (ndt.c:1925) and
 * flattens.  Returns 0, or -1 with a message in `err` when the scene cannot go to the device. */
int ndt_flatten_scene(scene *scn, ndt_flat_builder *fb, char *err, int err_len);
int ndt_flatten_scene_mt(scene *scn, ndt_flat_builder *fb, char *err, int err_len, int threads);
/* The same with the bounding-sphere fits delegated: `fit` takes a batch of point lists in the flat form of ndt_hip_fit_spheres
 * (include/ndt_hip.h) and returns 0 or, with the message in `err`, non-zero.  It is called at most three times a frame: (a) the
 * top-level objects before the kd build, (b) the kd items and hcube faces the loops would fit lazily, (c) the hcubes' own
 * spheres, which their faces reset.  fit == NULL: ndt_flatten_scene_mt.  `stats` (may be NULL) says what the frame fitted. */
typedef int (*ndt_fit_fn)(void *arg, int dims, int64_t n_lists, const int64_t *first, const double *points, const double *point_radius,
                          double *centers, double *radii, char *err, int err_len);
typedef struct {
    int64_t spheres;            /* objects whose sphere `fit` made */
    int64_t points;             /* bounding points handed to it */
    int calls;
    double gather_ms, fit_ms;   /* collecting the points (bounding_points of every object) / inside `fit`; without a fitter
                                 * fit_ms is the time of the host fits (points and search together) */
} ndt_fit_stats;
int ndt_flatten_scene_fit(scene *scn, ndt_flat_builder *fb, char *err, int err_len, int threads, ndt_fit_fn fit, void *fit_arg,
                          ndt_fit_stats *stats);
/* The same with the kd-tree build delegated as well: ndt_kd_add_object still makes the item boxes, `kd` gets them flat (the
 * arguments of ndt_hip_build_kdtree) exactly once a frame and returns the tree in malloc'ed arrays, which become the flat
 * scene's; 0 or, with the message in `err`, non-zero.  kd == NULL: ndt_kd_build.  The two delegations are independent.
 * `kd_stats` (may be NULL) says what the build cost, whoever made it. */
typedef int (*ndt_kd_fn)(void *arg, int dims, int n_items, const double *lower, const double *upper, const unsigned char *finite,
                         ndt_host_kdtree *out, char *err, int err_len);
typedef struct {
    double build_ms;            /* inside ndt_kd_build / inside `kd` */
    int calls;                  /* of `kd` */
} ndt_kd_stats;
int ndt_flatten_scene_with(scene *scn, ndt_flat_builder *fb, char *err, int err_len, int threads, ndt_fit_fn fit, void *fit_arg,
                           ndt_fit_stats *stats, ndt_kd_fn kd, void *kd_arg, ndt_kd_stats *kd_stats);
/* ndt_render.c: where the bounding spheres of the frames this process flattens for rendering are fitted -- 0 on the host
 * (default), 1 on the GPU (`ndt_hip --fit gpu`) -- and ndt_flatten_scene_fit with context 0 of the calling thread as the
 * fitter (the contexts are created first).  It prints `fitted K bounding spheres on GPU D in L launches`; there is no
 * fallback: without a device, or with a scene the device fit refuses, it fails with the reason in `err`. */
void ndt_render_fit_on_gpu(int on);
int ndt_flatten_scene_gpu_fit(scene *scn, ndt_flat_builder *fb, char *err, int err_len, int threads, ndt_fit_stats *stats);
/* ... and where their kd-trees are built -- 0 on the host (default), 1 on the GPU (`ndt_hip --kd gpu`, ndt_hip_build_kdtree on
 * context 0 of the calling thread) -- and the flattening with either piece, both or neither on the GPU.  With the tree on the
 * GPU it prints `built kd-tree of K nodes on GPU D in L launches`; no fallback either. */
void ndt_render_kd_on_gpu(int on);
int ndt_flatten_scene_gpu(scene *scn, ndt_flat_builder *fb, char *err, int err_len, int threads, int fit_on_gpu, int kd_on_gpu,
                          ndt_fit_stats *stats, ndt_kd_stats *kd_stats);
void ndt_flat_builder_free(ndt_flat_builder *fb);
int ndt_write_ndtscene(const ndt_flat_scene *fs, const char *name, const char *path);

#endif
