// ndt_kd.hip -- kd_tree_build (reference kd-tree.c:294-477) for the item boxes of a frame, on the device.
//
// The host builder (ndt_amd/host/src/ndt_kdtree.c) is the specification: the exhaustive split search, its candidate order and
// its first-strictly-best rule decide the tree, the tree decides pixels.  The only floating-point operations are
// `bound -/+ 2 EPSILON`, `candidate -/+ EPSILON` (one correctly rounded add each, -ffp-contract=off) and < / > on doubles;
// scores are integers.  So the device can afford the pass as the reference wrote it -- every candidate against every item of
// its node, inverted boxes through the same if / else-if -- and gets the same tree.
//
// Mapping.  The tree is built level by level; a level is three launches over all of its open nodes:
//   k_kd_score      the candidates of a node are ranked dimension-major, then by the item's place in the node's list, then lower
//                   bound before upper bound.  A node's candidates of one dimension are cut into slices of KD_SLICE; one
//                   wavefront scores a slice: a lane holds KD_CAND_LANE candidates in registers and the node's bounds in that
//                   dimension pass through LDS in tiles of KD_TILE items, read by all lanes at once.  The slice's best candidate
//                   -- the maximum of the packed key (score + n) << 32 | ~rank, i.e. the first of the best -- goes to the
//                   slice's own record with its two counts.  Small nodes are a wavefront per dimension, the root of the 8-D
//                   hypercube is 824 of them.
//   k_kd_plan       one workgroup: per node the best of its slices; a node with no valid candidate becomes a leaf.  The children's
//                   sizes follow from the winner's counts (left = n - right count, right = n - left count), so an exclusive scan
//                   over the level's nodes gives every child its node number, the place of its list and its first slice, and the
//                   totals of the next level, which the host reads back (24 bytes a level) to size the buffers BEFORE anything
//                   is written there.
//   k_kd_partition  one wavefront per split node walks the node's list 64 items at a time and appends to the two children's
//                   lists in the parent's order (ballot + popcount); straddlers go to both.
// No atomics, no workgroup waits for another, plain vector stores; the level loop on the host is bounded by NDT_KD_STACK.
//
// State.  Level-order nodes, one append-only array of item references (every node's list stays where it was written: a
// leaf's list is final), the slice records, two slice-offset arrays (this level's and the next's): grow-only buffers of the
// context.  Preorder numbering and the gathering of the leaf lists run on the host over the downloaded arrays.
#include "ndt_ctx.hpp"
#include <float.h>

namespace ndt_impl {

#define KD_CAND_LANE 2                      /* candidates a lane scores */
#define KD_SLICE (64 * KD_CAND_LANE)        /* candidates a wavefront scores */
#define KD_TILE 256                         /* items whose bounds stand in LDS at a time (4 KiB) */
#define KD_PLAN_THREADS 256                 /* the planning workgroup: KD_PLAN_THREADS / 64 wavefronts */
#define KD_MAX_REFS (1LL << 30)             /* item references the tree under construction may hold (4 GiB) */
#define KD_MAX_NODES (1LL << 26)
#define KD_MAX_SLICES (1LL << 30)

struct KdNode {             // a node of the tree under construction, in level order
    int dim;                // -2 not planned yet, -1 leaf, >= 0 split dimension
    int first, count;       // its list: refs[first .. first + count)
    int left;               // split: its children are the nodes left and left + 1
    double boundary;
};
struct KdSlice {            // the best candidate of a slice
    unsigned long long key; // 0: none is valid
    int left, right;        // its counts (kdtree_split_score's)
};

// slices a node of n items is scored in: none below two items (a valid candidate has an item on either side)
__host__ __device__ static inline long long kd_slices(int n, int dims)
{
    return n < 2 ? 0 : (long long)dims * ((2 * n + KD_SLICE - 1) / KD_SLICE);
}

__global__ __launch_bounds__(64) void k_kd_score(const KdNode *__restrict__ nodes, int node_begin, int n_nodes, const long long *__restrict__ slice_off,
                                                  const int *__restrict__ refs, const double *__restrict__ lower, const double *__restrict__ upper, int dims,
                                                  KdSlice *__restrict__ out)
{
    __shared__ double t_lo[KD_TILE], t_up[KD_TILE];
    const long long s = blockIdx.x;
    const int lane = (int)threadIdx.x;
    // the node of this slice: the last one whose first slice is not beyond s (nodes without slices share their successor's offset)
    int a = 0, b = n_nodes;
    while (b - a > 1) {
        const int mid = a + (b - a) / 2;
        if (slice_off[mid] <= s) a = mid; else b = mid;
    }
    const KdNode nd = nodes[node_begin + a];
    const int n = nd.count;
    const int per_dim = (2 * n + KD_SLICE - 1) / KD_SLICE;
    const int local = (int)(s - slice_off[a]);
    const int dim = local / per_dim, c0 = (local % per_dim) * KD_SLICE;
    if (n < 2 || dim >= dims) return;           // (cannot happen: the plan made the offsets from kd_slices)

    // kd_tree_split_node's candidates, kd-tree.c:330-360: lower bound - 2 EPSILON, upper bound + 2 EPSILON
    double x[KD_CAND_LANE], y[KD_CAND_LANE];
    int left[KD_CAND_LANE], right[KD_CAND_LANE];
#pragma unroll
    for (int k = 0; k < KD_CAND_LANE; ++k) {
        const int c = c0 + k * 64 + lane;
        double cand = 0.0;
        if (c < 2 * n) {
            const int id = refs[nd.first + (c >> 1)];
            cand = (c & 1) ? upper[(long long)id * dims + dim] + 2 * NDT_EPS : lower[(long long)id * dims + dim] - 2 * NDT_EPS;
        }
        x[k] = cand - NDT_EPS;
        y[k] = cand + NDT_EPS;
        left[k] = right[k] = 0;
    }
    // kdtree_split_score, kd-tree.c:294-313, over the node's list
    for (int t0 = 0; t0 < n; t0 += KD_TILE) {
        const int cnt = n - t0 < KD_TILE ? n - t0 : KD_TILE;
        __syncthreads();
        for (int j = lane; j < cnt; j += 64) {
            const int id = refs[nd.first + t0 + j];
            t_lo[j] = lower[(long long)id * dims + dim];
            t_up[j] = upper[(long long)id * dims + dim];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double lo = t_lo[j], up = t_up[j];
#pragma unroll
            for (int k = 0; k < KD_CAND_LANE; ++k) {
                if (up < x[k]) ++left[k];
                else if (lo > y[k]) ++right[k];
            }
        }
    }
    unsigned long long best = 0ull;
    int best_l = 0, best_r = 0;
#pragma unroll
    for (int k = 0; k < KD_CAND_LANE; ++k) {
        const int c = c0 + k * 64 + lane;
        if (c >= 2 * n || left[k] <= 0 || right[k] <= 0) continue;
        const int d = left[k] - right[k];
        const int score = n - ((d < 0 ? -d : d) + 2 * (n - left[k] - right[k]));
        const unsigned int rank = (unsigned int)dim * (unsigned int)(2 * n) + (unsigned int)c;
        const unsigned long long key = ((unsigned long long)(unsigned int)(score + n) << 32) | (unsigned long long)(0xffffffffu - rank);
        if (key > best) { best = key; best_l = left[k]; best_r = right[k]; }
    }
    unsigned long long top = best;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(top, off, 64);
        top = other > top ? other : top;
    }
    // (keys of valid candidates are distinct and non-zero: exactly one lane holds the winner)
    if (top == 0ull ? lane == 0 : best == top) {
        KdSlice r;
        r.key = top;
        r.left = top ? best_l : 0;
        r.right = top ? best_r : 0;
        out[s] = r;
    }
}

// totals[0..2]: nodes, item references and slices of the next level
__global__ __launch_bounds__(KD_PLAN_THREADS) void k_kd_plan(KdNode *__restrict__ nodes, int node_begin, int n_nodes, const long long *__restrict__ slice_off,
                                                   const KdSlice *__restrict__ slices, const int *__restrict__ refs, const double *__restrict__ lower,
                                                   const double *__restrict__ upper, int dims, int next_node_begin, long long next_ref_begin,
                                                   long long *__restrict__ next_slice_off, long long *__restrict__ totals)
{
    __shared__ long long wave_sum[KD_PLAN_THREADS / 64][3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry[3] = { 0, 0, 0 };
    for (int base = 0; base < n_nodes; base += KD_PLAN_THREADS) {
        const int j = base + tid;
        long long v[3] = { 0, 0, 0 };
        KdNode nd{};
        int nl = 0, nr = 0;
        if (j < n_nodes) {
            nd = nodes[node_begin + j];
            KdSlice bestc{ 0ull, 0, 0 };
            for (long long s = slice_off[j]; s < slice_off[j + 1]; ++s) {
                const KdSlice c = slices[s];
                if (c.key > bestc.key) bestc = c;
            }
            if (bestc.key) {
                const unsigned int rank = 0xffffffffu - (unsigned int)(bestc.key & 0xffffffffull);
                const unsigned int two_n = (unsigned int)(2 * nd.count);
                const int dim = (int)(rank / two_n), c = (int)(rank % two_n);
                const int id = refs[nd.first + (c >> 1)];
                nd.dim = dim;
                nd.boundary = (c & 1) ? upper[(long long)id * dims + dim] + 2 * NDT_EPS : lower[(long long)id * dims + dim] - 2 * NDT_EPS;
                nl = nd.count - bestc.right;        // the left items and the straddlers
                nr = nd.count - bestc.left;
                v[0] = 2;
                v[1] = (long long)nl + nr;
                v[2] = kd_slices(nl, dims) + kd_slices(nr, dims);
            } else {
                nd.dim = -1;
                nd.boundary = 0.0;
            }
        }
        // exclusive scan of v over the workgroup
        long long incl[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            long long t = v[q];
            for (int d = 1; d < 64; d <<= 1) {
                const long long up = __shfl_up(t, d, 64);
                if (lane >= d) t += up;
            }
            incl[q] = t;
        }
        __syncthreads();                            // (the previous round's readers of wave_sum are done)
        if (lane == 63)
            for (int q = 0; q < 3; ++q) wave_sum[wave][q] = incl[q];
        __syncthreads();
        long long before[3], total[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            long long bsum = 0, tsum = 0;
            for (int w = 0; w < KD_PLAN_THREADS / 64; ++w) {
                if (w < wave) bsum += wave_sum[w][q];
                tsum += wave_sum[w][q];
            }
            before[q] = carry[q] + bsum + incl[q] - v[q];
            total[q] = tsum;
        }
        if (j < n_nodes) {
            if (nd.dim >= 0) {
                const int child = next_node_begin + (int)before[0];
                nd.left = child;
                KdNode l{}, r{};
                l.dim = r.dim = -2;
                l.left = r.left = -1;
                l.first = (int)(next_ref_begin + before[1]);
                l.count = nl;
                r.first = (int)(next_ref_begin + before[1] + nl);
                r.count = nr;
                nodes[child] = l;
                nodes[child + 1] = r;
                next_slice_off[before[0]] = before[2];
                next_slice_off[before[0] + 1] = before[2] + kd_slices(nl, dims);
            } else {
                nd.left = -1;
            }
            nodes[node_begin + j] = nd;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) carry[q] += total[q];
    }
    if (tid == 0) {
        next_slice_off[carry[0]] = carry[2];
        totals[0] = carry[0];
        totals[1] = carry[1];
        totals[2] = carry[2];
    }
}

// kd_tree_split_node's partition, kd-tree.c:380-400: the same three-way test at the chosen (dim, boundary); both children keep
// the parent's order
__global__ __launch_bounds__(64) void k_kd_partition(const KdNode *__restrict__ nodes, int node_begin, int *refs, long long refs_cap,
                                                      const double *__restrict__ lower, const double *__restrict__ upper, int dims)
{
    const KdNode nd = nodes[node_begin + blockIdx.x];
    if (nd.dim < 0) return;
    const KdNode l = nodes[nd.left], r = nodes[nd.left + 1];
    const int lane = (int)threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const double x = nd.boundary - NDT_EPS, y = nd.boundary + NDT_EPS;
    int nl = 0, nr = 0;
    for (int base = 0; base < nd.count; base += 64) {
        const int i = base + lane;
        bool go_l = false, go_r = false;
        int id = 0;
        if (i < nd.count) {
            id = refs[nd.first + i];
            const double up = upper[(long long)id * dims + nd.dim], lo = lower[(long long)id * dims + nd.dim];
            if (up < x) go_l = true;
            else if (lo > y) go_r = true;
            else go_l = go_r = true;
        }
        const unsigned long long vl = __ballot(go_l), vr = __ballot(go_r);
        const int pl = nl + __popcll(vl & below), pr = nr + __popcll(vr & below);
        // (the counts are the plan's; the bounds are checked all the same: nothing is ever stored outside a child's list)
        if (go_l && pl < l.count && (long long)l.first + pl < refs_cap) refs[l.first + pl] = id;
        if (go_r && pr < r.count && (long long)r.first + pr < refs_cap) refs[r.first + pr] = id;
        nl += __popcll(vl);
        nr += __popcll(vr);
    }
}

void free_kd(ndt_hip_ctx *ctx)
{
    KdState &k = ctx->kd;
    void *bufs[] = { k.d_bounds, k.d_refs, k.d_nodes, k.d_slices, k.d_slice_off[0], k.d_slice_off[1], k.d_totals };
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    k = KdState();
}

// Makes *p hold at least `need` bytes, keeping its first `keep` bytes.  Growth policy: nothing is allocated ahead of need
// except by doubling -- the new size is max(need, 2 * old size).
static int kd_grow(ndt_hip_ctx *ctx, void **p, size_t *cap, size_t need, size_t keep, const char *what)
{
    if (need <= *cap) return NDT_OK;
    const size_t want = need > 2 * *cap ? need : 2 * *cap;
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, want);
    if (e != hipSuccess) return fail(NDT_E_NOMEM, "ndt_hip_build_kdtree: %s need %zu bytes: hipMalloc: %s", what, want, hipGetErrorString(e));
    if (*p) {
        if (keep > 0) e = hipMemcpyAsync(q, *p, keep, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(q);
            return fail(NDT_E_DEVICE, "ndt_hip_build_kdtree: moving %s: %s", what, hipGetErrorString(e));
        }
        (void)hipFree(*p);
        ctx->kd.grows += 1;
    }
    *p = q;
    *cap = want;
    return NDT_OK;
}

#define KD_TRY(expr)                    \
    do {                                \
        const int rc_ = (expr);         \
        if (rc_ != NDT_OK) return rc_;  \
    } while (0)

int build_kdtree_device(ndt_hip_ctx *ctx, int dims, int n_items, const double *lower, const double *upper, const unsigned char *finite)
{
    KdState &k = ctx->kd;
    k.valid = false;
    k.launches = 0;
    k.grows = 0;
    k.depth = 0;
    k.dims = dims;
    // kd_tree_build, kd-tree.c:421-477: the finite items in id order are the root's list, the others are kept apart; the root
    // box grows by compare-and-assign (aabb_add, kd-tree.c:42-61)
    std::vector<int> root;
    k.inf_refs.clear();
    k.bb_lower.assign((size_t)dims, DBL_MAX);
    k.bb_upper.assign((size_t)dims, -DBL_MAX);
    for (int i = 0; i < n_items; ++i) {
        if (!finite[i]) { k.inf_refs.push_back(i); continue; }
        root.push_back(i);
        for (int d = 0; d < dims; ++d) {
            if (lower[(size_t)i * dims + d] < k.bb_lower[(size_t)d]) k.bb_lower[(size_t)d] = lower[(size_t)i * dims + d];
            if (upper[(size_t)i * dims + d] > k.bb_upper[(size_t)d]) k.bb_upper[(size_t)d] = upper[(size_t)i * dims + d];
        }
    }
    const int nf = (int)root.size();

    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t box_bytes = sizeof(double) * (size_t)(n_items > 0 ? n_items : 1) * dims;
    KD_TRY(kd_grow(ctx, &k.d_bounds, &k.bounds_bytes, 2 * box_bytes, 0, "the item boxes"));
    KD_TRY(kd_grow(ctx, &k.d_refs, &k.refs_bytes, sizeof(int) * (4 * (size_t)nf + 1024), 0, "the item references"));
    KD_TRY(kd_grow(ctx, &k.d_nodes, &k.nodes_bytes, sizeof(KdNode) * 1024, 0, "the nodes"));
    KD_TRY(kd_grow(ctx, &k.d_totals, &k.totals_bytes, 3 * sizeof(long long), 0, "the level totals"));
    double *d_lower = (double *)k.d_bounds, *d_upper = (double *)((char *)k.d_bounds + box_bytes);
    if (n_items > 0) {
        HIP_TRY(hipMemcpyAsync(d_lower, lower, sizeof(double) * (size_t)n_items * dims, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_upper, upper, sizeof(double) * (size_t)n_items * dims, hipMemcpyHostToDevice, s));
    }
    if (nf > 0) HIP_TRY(hipMemcpyAsync(k.d_refs, root.data(), sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, s));
    KdNode root_node{};
    root_node.dim = -2;
    root_node.first = 0;
    root_node.count = nf;
    root_node.left = -1;
    HIP_TRY(hipMemcpyAsync(k.d_nodes, &root_node, sizeof(KdNode), hipMemcpyHostToDevice, s));
    long long first_off[2] = { 0, kd_slices(nf, dims) };
    KD_TRY(kd_grow(ctx, &k.d_slice_off[0], &k.slice_off_bytes[0], sizeof(first_off), 0, "the slice offsets"));
    HIP_TRY(hipMemcpyAsync(k.d_slice_off[0], first_off, sizeof(first_off), hipMemcpyHostToDevice, s));

    long long node_begin = 0, nn = 1, refs_end = nf, n_slices = first_off[1];
    int cur = 0, depth = 0;
    long long *h_totals = (long long *)ctx->h_counters;         // pinned; this call is synchronous on the context
    for (int lvl = 0; lvl < NDT_KD_STACK; ++lvl) {
        depth = lvl + 1;
        // what this level's plan may write: two children a node, their slice offsets and one more
        if (node_begin + 3 * nn > KD_MAX_NODES)
            return fail(NDT_E_NOMEM, "ndt_hip_build_kdtree: level %d needs room for %lld nodes (limit %lld)", lvl, node_begin + 3 * nn, (long long)KD_MAX_NODES);
        KD_TRY(kd_grow(ctx, &k.d_nodes, &k.nodes_bytes, sizeof(KdNode) * (size_t)(node_begin + 3 * nn), sizeof(KdNode) * (size_t)(node_begin + nn), "the nodes"));
        KD_TRY(kd_grow(ctx, &k.d_slice_off[cur ^ 1], &k.slice_off_bytes[cur ^ 1], sizeof(long long) * (size_t)(2 * nn + 1), 0, "the slice offsets"));
        KD_TRY(kd_grow(ctx, &k.d_slices, &k.slices_bytes, sizeof(KdSlice) * (size_t)(n_slices > 0 ? n_slices : 1), 0, "the slice records"));
        if (n_slices > 0) {
            hipLaunchKernelGGL(k_kd_score, dim3((unsigned)n_slices), dim3(64), 0, s, (const KdNode *)k.d_nodes, (int)node_begin, (int)nn,
                               (const long long *)k.d_slice_off[cur], (const int *)k.d_refs, d_lower, d_upper, dims, (KdSlice *)k.d_slices);
            HIP_TRY(hipGetLastError());
            k.launches += 1;
        }
        hipLaunchKernelGGL(k_kd_plan, dim3(1), dim3(KD_PLAN_THREADS), 0, s, (KdNode *)k.d_nodes, (int)node_begin, (int)nn, (const long long *)k.d_slice_off[cur],
                           (const KdSlice *)k.d_slices, (const int *)k.d_refs, d_lower, d_upper, dims, (int)(node_begin + nn), refs_end,
                           (long long *)k.d_slice_off[cur ^ 1], (long long *)k.d_totals);
        HIP_TRY(hipGetLastError());
        k.launches += 1;
        HIP_TRY(hipMemcpyAsync(h_totals, k.d_totals, 3 * sizeof(long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const long long next_nodes = h_totals[0], next_refs = h_totals[1], next_slices = h_totals[2];
        if (next_nodes == 0) break;
        if (lvl + 2 > NDT_KD_STACK)
            return fail(NDT_E_UNSUPPORTED, "ndt_hip_build_kdtree: the kd-tree is deeper than %d levels, the depth the traversal stack holds (%d)", lvl + 1, NDT_KD_STACK);
        if (refs_end + next_refs > KD_MAX_REFS || next_slices > KD_MAX_SLICES)
            return fail(NDT_E_NOMEM, "ndt_hip_build_kdtree: level %d needs %lld item references and %lld slices (limits %lld, %lld)", lvl + 1,
                        refs_end + next_refs, next_slices, (long long)KD_MAX_REFS, (long long)KD_MAX_SLICES);
        KD_TRY(kd_grow(ctx, &k.d_refs, &k.refs_bytes, sizeof(int) * (size_t)(refs_end + next_refs), sizeof(int) * (size_t)refs_end, "the item references"));
        hipLaunchKernelGGL(k_kd_partition, dim3((unsigned)nn), dim3(64), 0, s, (const KdNode *)k.d_nodes, (int)node_begin, (int *)k.d_refs,
                           (long long)(k.refs_bytes / sizeof(int)), d_lower, d_upper, dims);
        HIP_TRY(hipGetLastError());
        k.launches += 1;
        node_begin += nn;
        nn = next_nodes;
        refs_end += next_refs;
        n_slices = next_slices;
        cur ^= 1;
    }

    // the tree in level order and every node's list
    const long long n_nodes = node_begin + nn;
    std::vector<KdNode> lv((size_t)n_nodes);
    std::vector<int> refs((size_t)(refs_end > 0 ? refs_end : 1));
    HIP_TRY(hipMemcpyAsync(lv.data(), k.d_nodes, sizeof(KdNode) * (size_t)n_nodes, hipMemcpyDeviceToHost, s));
    if (refs_end > 0) HIP_TRY(hipMemcpyAsync(refs.data(), k.d_refs, sizeof(int) * (size_t)refs_end, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // preorder, as flatten_node numbers the host tree: a node, its left subtree, its right subtree
    k.nodes.clear();
    k.nodes.reserve((size_t)n_nodes);
    k.leaf_refs.clear();
    bool sound = true;
    std::function<void(long long)> visit = [&](long long at) {
        const KdNode &nd = lv[(size_t)at];
        const size_t me = k.nodes.size();
        ndt_flat_kdnode f;
        memset(&f, 0, sizeof(f));
        f.dim = nd.dim;
        k.nodes.push_back(f);
        if (nd.dim >= 0) {
            if (nd.left <= at || (long long)nd.left + 1 >= n_nodes) { sound = false; return; }
            k.nodes[me].boundary = nd.boundary;
            k.nodes[me].left = (int32_t)me + 1;
            visit(nd.left);
            k.nodes[me].right = (int32_t)k.nodes.size();
            visit((long long)nd.left + 1);
        } else {
            if (nd.dim != -1 || nd.first < 0 || nd.count < 0 || (long long)nd.first + nd.count > refs_end) { sound = false; return; }
            k.nodes[me].left = k.nodes[me].right = -1;
            k.nodes[me].first = (int32_t)k.leaf_refs.size();
            k.nodes[me].num = nd.count;
            k.leaf_refs.insert(k.leaf_refs.end(), refs.begin() + nd.first, refs.begin() + nd.first + nd.count);
        }
    };
    visit(0);
    if (!sound || (long long)k.nodes.size() != n_nodes)
        return fail(NDT_E_DEVICE, "ndt_hip_build_kdtree: the device returned an inconsistent tree");
    if (k.leaf_refs.size() > 0x7fffffffull) return fail(NDT_E_NOMEM, "ndt_hip_build_kdtree: %zu leaf references do not fit the flat scene", k.leaf_refs.size());
    k.depth = depth;
    k.valid = true;
    return NDT_OK;
}

} // namespace ndt_impl

// ------------------------------------------------------------------ the C ABI

extern "C" int ndt_hip_build_kdtree(ndt_hip_ctx *ctx, int32_t dims, int32_t n_items, const double *lower, const double *upper,
                                    const uint8_t *finite, ndt_kd_counts *counts)
{
    if (ctx) ctx->kd.valid = false;
    if (dims < NDT_MIN_DIMS || dims > NDT_MAX_DIMS)
        return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: dims = %d: the builder takes %d..%d dimensions", dims, NDT_MIN_DIMS, NDT_MAX_DIMS);
    if (n_items < 0) return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: n_items = %d is negative", n_items);
    if (n_items > (1 << 26)) return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: n_items = %d: at most %d items", n_items, 1 << 26);
    if (n_items > 0 && !lower) return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: lower is NULL");
    if (n_items > 0 && !upper) return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: upper is NULL");
    if (n_items > 0 && !finite) return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: finite is NULL");
    if (!counts) return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: counts is NULL");
    if (!ctx) return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: ctx is NULL");
    memset(counts, 0, sizeof(*counts));
    for (long long i = 0; i < (long long)n_items * dims; ++i)
        if (lower[i] != lower[i] || upper[i] != upper[i])
            return fail(NDT_E_INVALID, "ndt_hip_build_kdtree: item %lld has a NaN bound (the caller builds those itself)", i / dims);
    const int rc = build_kdtree_device(ctx, dims, n_items, lower, upper, finite);
    counts->launches = ctx->kd.launches;
    counts->grows = ctx->kd.grows;
    if (rc != NDT_OK) return rc;
    counts->n_kd_nodes = (int32_t)ctx->kd.nodes.size();
    counts->n_leaf_refs = (int32_t)ctx->kd.leaf_refs.size();
    counts->n_inf = (int32_t)ctx->kd.inf_refs.size();
    counts->depth = ctx->kd.depth;
    return NDT_OK;
}

extern "C" int ndt_hip_kdtree_fetch(ndt_hip_ctx *ctx, ndt_flat_kdnode *nodes, int32_t *leaf_refs, int32_t *inf_refs, double *bb_lower, double *bb_upper)
{
    if (!ctx) return fail(NDT_E_INVALID, "ndt_hip_kdtree_fetch: ctx is NULL");
    const KdState &k = ctx->kd;
    if (!k.valid) return fail(NDT_E_STATE, "ndt_hip_kdtree_fetch: the context holds no kd-tree (no build yet, or the last one failed)");
    if (!nodes || !bb_lower || !bb_upper || (!leaf_refs && !k.leaf_refs.empty()) || (!inf_refs && !k.inf_refs.empty()))
        return fail(NDT_E_INVALID, "ndt_hip_kdtree_fetch: NULL array");
    memcpy(nodes, k.nodes.data(), k.nodes.size() * sizeof(ndt_flat_kdnode));
    if (!k.leaf_refs.empty()) memcpy(leaf_refs, k.leaf_refs.data(), k.leaf_refs.size() * sizeof(int32_t));
    if (!k.inf_refs.empty()) memcpy(inf_refs, k.inf_refs.data(), k.inf_refs.size() * sizeof(int32_t));
    memcpy(bb_lower, k.bb_lower.data(), (size_t)k.dims * sizeof(double));
    memcpy(bb_upper, k.bb_upper.data(), (size_t)k.dims * sizeof(double));
    return NDT_OK;
}

extern "C" int ndt_hip_kd_launches(ndt_hip_ctx *ctx) { return ctx ? ctx->kd.launches : 0; }
