/* ndt_bounding.c -- bounding-sphere lists and the minimum enclosing sphere fit
 * (reference bounding.c:89-240), restated. */
#include "ndt_host_api.h"

int bounds_list_init(bounds_list *list)
{
    list->head = list->tail = NULL;
    return 0;
}

/* new nodes go to the FRONT (bounding.c:94-112): list order affects the centroid's rounding
 * and through it the Nelder-Mead seed */
int bounds_list_add(bounds_list *list, vectNd *vect, double radius)
{
    bounds_node *node = (bounds_node *)calloc(1, sizeof(bounds_node));
    if (!node) { perror("calloc"); exit(1); }
    node->next = list->head;
    list->head = node;
    if (!list->tail) list->tail = node;
    vectNd_calloc(&node->bounds.center, vect->n);
    vectNd_copy(&node->bounds.center, vect);
    node->bounds.radius = radius;
    return 0;
}

int bounds_list_join(bounds_list *list, bounds_list *other)
{
    if (list->tail) list->tail->next = other->head;
    else list->head = other->head;
    list->tail = other->tail;
    other->head = other->tail = NULL;
    return 0;
}

int bounds_list_free(bounds_list *list)
{
    for (bounds_node *n = list->head; n;) {
        bounds_node *next = n->next;
        vectNd_free(&n->bounds.center);
        free(n);
        n = next;
    }
    list->head = list->tail = NULL;
    return 0;
}

int bounds_list_centroid(bounds_list *list, vectNd *centroid)
{
    vectNd sum;
    int count = 0;
    vectNd_calloc(&sum, centroid->n);
    for (bounds_node *n = list->head; n; n = n->next) {
        vectNd_add(&sum, &n->bounds.center, &sum);
        ++count;
    }
    vectNd_scale(&sum, 1.0 / count, centroid);
    vectNd_free(&sum);
    return 0;
}

int bounds_list_radius(bounds_list *list, vectNd *centroid, double *radius)
{
    double max = -1.0;
    for (bounds_node *n = list->head; n; n = n->next) {
        double dist = -1.0;
        vectNd_dist(centroid, &n->bounds.center, &dist);
        if (n->bounds.radius > 0.0) dist += n->bounds.radius;
        max = (dist > max) ? dist : max;
    }
    *radius = max;
    return 0;
}

/* bounding.c:177-240: Nelder-Mead over the centre, seeded with the centroid, at most 1000
 * iterations or until the simplex is smaller than EPSILON; the centroid wins if the search
 * ends worse than it started */
static int fit_optimal(bounds_list *list, vectNd *centroid, double *radius, int *evaluations, int *centroid_won)
{
    int dim = centroid->n;
    int n_results = 0, won = 0;
    void *nm = NULL;
    double curr_radius = -1.0;
    vectNd curr, initial;
    nm_init(&nm, dim);
    vectNd_calloc(&curr, dim);
    bounds_list_centroid(list, &curr);
    bounds_list_radius(list, &curr, &curr_radius);
    nm_set_seed(nm, &curr);
    vectNd_calloc(&initial, dim);
    vectNd_copy(&initial, &curr);
    const double initial_radius = curr_radius;
    while (!nm_done(nm, EPSILON, 1000)) {
        nm_add_result(nm, &curr, curr_radius);
        ++n_results;
        nm_next_point(nm, &curr);
        bounds_list_radius(list, &curr, &curr_radius);
    }
    nm_best_point(nm, &curr);
    bounds_list_radius(list, &curr, &curr_radius);
    if (curr_radius - initial_radius > EPSILON) {
        vectNd_copy(&curr, &initial);
        bounds_list_radius(list, &curr, &curr_radius);
        won = 1;
    }
    vectNd_copy(centroid, &curr);
    *radius = curr_radius;
    vectNd_free(&initial);
    vectNd_free(&curr);
    nm_free(nm);
    if (evaluations) *evaluations = n_results;
    if (centroid_won) *centroid_won = won;
    return 0;
}

int bounds_list_optimal(bounds_list *list, vectNd *centroid, double *radius)
{
    return fit_optimal(list, centroid, radius, NULL, NULL);
}

/* bounds_list_optimal for n_lists point lists given flat -- the signature of ndt_hip_fit_spheres (include/ndt_hip.h), run
 * through the functions above on the CPU: list i is points first[i] .. first[i+1] of points[.][dims] / point_radius[.] in
 * the order the list is walked, head first.  The twin the device fit is compared against.  Returns 0, or -1 for an
 * argument the device call refuses as well (dims < 1, an empty list).  _traced also tells, per list (either may be NULL),
 * how many results the search took (1 001: it ran into the iteration limit) and whether the centroid won in the end. */
int ndt_host_fit_spheres(int dims, int64_t n_lists, const int64_t *first, const double *points, const double *point_radius,
                         double *centers, double *radii)
{
    return ndt_host_fit_spheres_traced(dims, n_lists, first, points, point_radius, centers, radii, NULL, NULL);
}

int ndt_host_fit_spheres_traced(int dims, int64_t n_lists, const int64_t *first, const double *points, const double *point_radius,
                                double *centers, double *radii, int32_t *evaluations, int32_t *centroid_won)
{
    if (dims < 1 || n_lists < 0 || !first) return -1;
    vectNd p, c;
    vectNd_calloc(&p, dims);
    vectNd_calloc(&c, dims);
    int rc = 0;
    for (int64_t i = 0; i < n_lists && rc == 0; ++i) {
        if (first[i + 1] <= first[i]) { rc = -1; break; }
        bounds_list pts;
        bounds_list_init(&pts);
        for (int64_t k = first[i + 1] - 1; k >= first[i]; --k) {       /* bounds_list_add prepends: last point first */
            memcpy(p.v, points + k * dims, (size_t)dims * sizeof(double));
            bounds_list_add(&pts, &p, point_radius[k]);
        }
        int n_results = 0, won = 0;
        fit_optimal(&pts, &c, &radii[i], &n_results, &won);
        if (evaluations) evaluations[i] = n_results;
        if (centroid_won) centroid_won[i] = won;
        memcpy(centers + i * dims, c.v, (size_t)dims * sizeof(double));
        bounds_list_free(&pts);
    }
    vectNd_free(&p);
    vectNd_free(&c);
    return rc;
}

/* bounding.c:34-85.  Host copy of the gate the device evaluates per ray. */
int vect_bounding_sphere_intersect(bounding_sphere *sph, vectNd *o, vectNd *v, double min_dist)
{
    if (!sph->prepared) {
        sph->radius_sqr = sph->radius * sph->radius;
        sph->prepared = 1;
    }
    vectNd oc;
    double oc_len2, voc;
    vectNd_alloc(&oc, o->n);
    vectNd_sub(o, &sph->center, &oc);
    vectNd_dot(&oc, &oc, &oc_len2);
    if (min_dist > 0) {
        double reach = min_dist + sph->radius;
        if (oc_len2 > reach * reach) {
            vectNd_free(&oc);
            return 0;
        }
    }
    vectNd_dot(v, &oc, &voc);
    vectNd_free(&oc);
    double voc2 = voc * voc;
    double desc = voc2 - oc_len2 + sph->radius_sqr;
    if (desc < 0.0 || (voc > 0.0 && voc2 > desc)) return 0;
    return 1;
}
