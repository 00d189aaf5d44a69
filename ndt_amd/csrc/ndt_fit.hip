// ndt_fit.hip -- bounds_list_optimal (reference bounding.c:177-240) for a batch of point lists, on the device.
//
// A frame needs one bounding sphere per object and per nested hcube face before it can be uploaded: one Nelder-Mead
// search each (host: ndt_bounding.c:77, ndt_nelder_mead.c), thousands of small, independent, identical FP64 searches
// made of + - * /, sqrt and comparisons -- every one of them correctly rounded on gfx950 with -ffp-contract=off.  The
// kernel below restates the host files operation for operation, so a fit returns the 64-bit patterns the host returns.
//
// Mapping.  A fit is run by a group of 2^g lanes of one wavefront (g = 0 .. 6, chosen per launch from the length of the
// lists it takes: fit_lg_lanes).  The search is sequential and every lane of a group carries the whole state machine, so the
// lanes of a group are in the same state at every step; only the evaluation -- "largest distance to the bounding points",
// bounds_list_radius -- is shared out: lane j takes points j, j + 2^g, ... and the group reduces with a butterfly.  A
// radius is a MAXIMUM of independently computed doubles, and `dist > max ? dist : max` over non-NaN values gives the same
// bits in any order.  The centroid is a SUM: every lane adds it up itself, in list order.
//
// The simplex (N+1 points of N doubles, their values, x_r and the second shrink point) is indexed by rank, i.e.
// dynamically: it lives in LDS, one column per group, word-major across the groups of the block (word w of group q at
// lds[w * groups + q]: with one fit per lane the 64 lanes of an access hit 64 consecutive doubles).  All lanes of a group
// store the same values to the same words and read back what they stored themselves, so no lane depends on another
// lane's store and the kernel has no barrier.  The sort moves 4-bit slot numbers inside one 64-bit register, as the host
// sort moves pointers (ndt_nelder_mead.c:36-47).
//
// The loop is bounded by construction: the reference stops after 1 001 results (nm_done: iterations > 1000); the device
// loop has that trip count as a hard bound.  No atomics, nothing crosses a workgroup, plain vector stores.
#include "ndt_ctx.hpp"
#include <algorithm>

namespace ndt_impl {

struct FitJob {
    long long first;        // the list's first point in points[] / point_radius[]
    int count;              // its points (>= 1)
    int list;               // where its sphere goes in centers[] / radii[]
};

enum { NM_INITIAL = 0, NM_REFLECT, NM_EXPAND, NM_CONTRACT_OUT, NM_CONTRACT_IN, NM_SHRINK, NM_SHRINK2 };   // ndt_nelder_mead.c:10

// 8-byte words of LDS a fit keeps: simplex[N+1].x, simplex[N+1].f, xr.x, s_shrink (ndt_nelder_mead.c:17-25; x_e and x_c
// are only ever read in the call that sets them from the point just evaluated, which is in registers)
template <int N> struct FitWords {
    static constexpr int X = 0, F = (N + 1) * N, XR = F + N + 1, SS = XR + N, TOTAL = SS + N;
};

#define NDT_FIT_MAX_TRIPS 1002      /* 1 001 results (nm_done, ndt_nelder_mead.c:226) + the check that ends the search */

template <int N>
__global__ __launch_bounds__(64) void k_fit(const FitJob *__restrict__ jobs, int n_jobs, int lg_lanes, const double *__restrict__ points,
                                             const double *__restrict__ point_radius, double *__restrict__ centers, double *__restrict__ radii)
{
    extern __shared__ double fit_lds[];
    typedef FitWords<N> W;
    const int lanes = 1 << lg_lanes, groups = 64 >> lg_lanes;
    const int group = (int)threadIdx.x >> lg_lanes, sub = (int)threadIdx.x & (lanes - 1);
    const long long job = (long long)blockIdx.x * groups + group;
    if (job >= n_jobs) return;          // (whole groups leave: the butterfly below never looks outside its group)
    const FitJob jb = jobs[job];
    const int cnt = jb.count;
    const double *P = points + jb.first * N, *R = point_radius + jb.first;
    double *const col = fit_lds + group;
#define LDS(w) col[(w) * groups]

    // bounds_list_radius, ndt_bounding.c:61-72
    auto list_radius = [&](const double (&c)[N]) -> double {
        double max = -1.0;
        for (int p = sub; p < cnt; p += lanes) {
            double pt[N], d[N];
#pragma unroll
            for (int k = 0; k < N; ++k) pt[k] = P[(long long)p * N + k];
            v_sub<N>(c, pt, d);                                 // vectNd_dist(centroid, point): centroid - point
            double dist = sqrt(v_dot<N>(d, d));
            const double r = R[p];
            if (r > 0.0) dist += r;
            max = (dist > max) ? dist : max;
        }
        for (int off = lanes >> 1; off > 0; off >>= 1) {
            const double other = __shfl_xor(max, off, 64);
            max = (other > max) ? other : max;
        }
        return max;
    };

    // bounds_list_centroid, ndt_bounding.c:47-59: running sum in list order, then * (1.0 / count)
    double curr[N], seed[N], initial[N];
    {
        double sum[N];
        v_zero<N>(sum);
        for (int p = 0; p < cnt; ++p) {
#pragma unroll
            for (int k = 0; k < N; ++k) sum[k] = sum[k] + P[(long long)p * N + k];
        }
        v_scale<N>(sum, 1.0 / cnt, curr);
    }
    double curr_radius = list_radius(curr);                     // ndt_bounding.c:86
    v_copy<N>(seed, curr);                                      // nm_set_seed, ndt_bounding.c:87
    v_copy<N>(initial, curr);
    const double initial_radius = curr_radius;

    // nm_init, ndt_nelder_mead.c:49-63.  rank -> slot of the simplex, 4 bits each (N + 1 <= 13 ranks)
    unsigned long long perm = 0xfedcba9876543210ull;
    int state = NM_INITIAL, iterations = 0, count = 0;
    double xr_f = 0.0;
    bool sorted = false;        // the simplex is in ascending order: sorting it again would move nothing
#define SLOT(rank) ((int)((perm >> (4 * (rank))) & 15ull))
#define SET_SLOT(rank, s) (perm = (perm & ~(15ull << (4 * (rank)))) | ((unsigned long long)(s) << (4 * (rank))))

    // nm_sort, ndt_nelder_mead.c:36-47: ascending by value, stable
    auto nm_sort = [&]() {
        if (sorted) return;
        for (int i = 1; i < count; ++i) {
            const int key = SLOT(i);
            const double key_f = LDS(W::F + key);
            int j = i - 1;
            while (j >= 0 && LDS(W::F + SLOT(j)) > key_f) {
                SET_SLOT(j + 1, SLOT(j));
                --j;
            }
            SET_SLOT(j + 1, key);
        }
        sorted = true;
    };
    // pt_set on simplex[rank], ndt_nelder_mead.c:28-32
    auto set_simplex = [&](int rank, const double (&x)[N], double f) {
        const int s = SLOT(rank);
#pragma unroll
        for (int k = 0; k < N; ++k) LDS(W::X + s * N + k) = x[k];
        LDS(W::F + s) = f;
        sorted = false;
    };

    // nm_add_result, ndt_nelder_mead.c:89-155
    auto nm_add_result = [&](const double (&x)[N], double value) {
        const int last = N;
        iterations += 1;
        if (state == NM_SHRINK2) {                              // :96-100
            set_simplex(count - 2, x, value);
            state = NM_REFLECT;
            return;
        }
        if (state == NM_SHRINK) {                               // :101-105
            set_simplex(count - 1, x, value);
            state = NM_SHRINK2;
            return;
        }
        if (count <= N) {                                       // :107-112
            set_simplex(count, x, value);
            count += 1;
            if (count >= N + 1) state = NM_REFLECT;
            return;
        }
        nm_sort();                                              // :113
        const double fh = LDS(W::F + SLOT(last)), fs = LDS(W::F + SLOT(last - 1)), fl = LDS(W::F + SLOT(0));
        const double fr = value;
        if (state == NM_REFLECT) {                              // :117-123
#pragma unroll
            for (int k = 0; k < N; ++k) LDS(W::XR + k) = x[k];
            xr_f = value;
            if (fl <= xr_f && xr_f < fs) {
                set_simplex(last, x, value);
                return;
            }
        }
        if (state == NM_EXPAND) {                               // :124-130 (x_e is x)
            if (value < xr_f) set_simplex(last, x, value);
            else {
                double xr[N];
#pragma unroll
                for (int k = 0; k < N; ++k) xr[k] = LDS(W::XR + k);
                set_simplex(last, xr, xr_f);
            }
            state = NM_REFLECT;
            return;
        }
        if (state == NM_CONTRACT_OUT) {                         // :131-138 (x_c is x)
            if (value < xr_f) {
                set_simplex(last, x, value);
                state = NM_REFLECT;
                return;
            }
        }
        if (state == NM_CONTRACT_IN) {                          // :139-146
            if (value < fh) {
                set_simplex(last, x, value);
                state = NM_REFLECT;
                return;
            }
        }
        if (fr < fl) state = NM_EXPAND;                         // :148-154
        else if (fr >= fs) state = (fs <= fr && fr < fh) ? NM_CONTRACT_OUT : NM_CONTRACT_IN;
        else state = NM_SHRINK;
    };

    // nm_next_point, ndt_nelder_mead.c:157-211
    auto nm_next_point = [&](double (&x)[N]) {
        if (state == NM_INITIAL && count < N + 1) {             // :161-170: the seed, then seed + k * e_(k-1)
#pragma unroll
            for (int k = 0; k < N; ++k) {
                x[k] = seed[k];
                if (k == count - 1) x[k] += count;
            }
            return;
        }
        if (count != N + 1) {                                   // :171-174
            v_copy<N>(x, seed);
            return;
        }
        if (state != NM_SHRINK && state != NM_SHRINK2) nm_sort();
        const int h = SLOT(N) * N, s = SLOT(N - 1) * N;
        if (state == NM_SHRINK) {                               // :200-204: towards x_r, not towards the best point
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double xr = LDS(W::XR + k);
                LDS(W::SS + k) = (xr + LDS(W::X + s + k)) * 0.5;
                x[k] = (xr + LDS(W::X + h + k)) * 0.5;
            }
            return;
        }
        if (state == NM_SHRINK2) {                              // :205-208
#pragma unroll
            for (int k = 0; k < N; ++k) {
                x[k] = LDS(W::SS + k);
                LDS(W::SS + k) = 0.0;
            }
            return;
        }
        // :178-183: centroid of all points but the worst, running sum from zero in rank order, then * 1/d
        double c[N];
        v_zero<N>(c);
        for (int i = 0; i < count - 1; ++i) {
            const int at = SLOT(i) * N;
#pragma unroll
            for (int k = 0; k < N; ++k) c[k] = c[k] + LDS(W::X + at + k);
        }
        const double inv = 1.0 / (count - 1);
        v_scale<N>(c, inv, c);
        const double alpha = 1, beta = 0.5, gamma = 2;          // :54
        if (state == NM_REFLECT) {                              // :188-190
#pragma unroll
            for (int k = 0; k < N; ++k) x[k] = c[k] + (c[k] - LDS(W::X + h + k)) * alpha;
        } else if (state == NM_EXPAND) {                        // :191-193
#pragma unroll
            for (int k = 0; k < N; ++k) x[k] = c[k] + (LDS(W::XR + k) - c[k]) * gamma;
        } else if (state == NM_CONTRACT_OUT) {                  // :194-196
#pragma unroll
            for (int k = 0; k < N; ++k) x[k] = c[k] + (LDS(W::XR + k) - c[k]) * beta;
        } else if (state == NM_CONTRACT_IN) {                   // :197-199
#pragma unroll
            for (int k = 0; k < N; ++k) x[k] = c[k] + (LDS(W::X + h + k) - c[k]) * beta;
        }
    };

    // ndt_bounding.c:91-95
    for (int trip = 0; trip < NDT_FIT_MAX_TRIPS; ++trip) {
        // nm_done(nm, EPSILON, 1000), ndt_nelder_mead.c:222-239
        if (state != NM_INITIAL) {
            if (iterations > 1000) break;
            if (state != NM_SHRINK && state != NM_SHRINK2) nm_sort();
            const int a = SLOT(0) * N, b = SLOT(count - 1) * N;
            double d[N];
#pragma unroll
            for (int k = 0; k < N; ++k) d[k] = LDS(W::X + a + k) - LDS(W::X + b + k);
            if (sqrt(v_dot<N>(d, d)) < NDT_EPS) break;
        }
        nm_add_result(curr, curr_radius);
        nm_next_point(curr);
        curr_radius = list_radius(curr);
    }

    // nm_best_point, ndt_nelder_mead.c:80-87
    {
        int best = 0;
        for (int i = 0; i < count; ++i)
            if (LDS(W::F + SLOT(i)) < LDS(W::F + SLOT(best))) best = i;
        if (best < count) {
            const int at = SLOT(best) * N;
#pragma unroll
            for (int k = 0; k < N; ++k) curr[k] = LDS(W::X + at + k);
        }
    }
    curr_radius = list_radius(curr);
    if (curr_radius - initial_radius > NDT_EPS) {               // ndt_bounding.c:98-101: the centroid wins
        v_copy<N>(curr, initial);
        curr_radius = list_radius(curr);
    }
    if (sub == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) centers[(long long)jb.list * N + k] = curr[k];
        radii[jb.list] = curr_radius;
    }
#undef LDS
#undef SLOT
#undef SET_SLOT
}

// lanes (as a power of two) that share a fit of `count` points: about four points a lane, one fit per lane up to four points
static int fit_lg_lanes(int count)
{
    int lg = 0;
    while (lg < 6 && (4 << lg) < count) ++lg;
    return lg;
}

template <int N> static hipError_t launch_fit(hipStream_t s, const FitJob *jobs, int n_jobs, int lg, const double *points, const double *prad,
                                              double *centers, double *radii)
{
    // one wavefront a workgroup; its LDS is what its 64 >> lg fits need: 193 words a fit at N = 12, 96.5 KiB for 64 of them.
    // More than 64 KiB of dynamic LDS has to be asked for (per device: asked at every launch, the call is a table look-up).
    hipError_t e = hipFuncSetAttribute((const void *)k_fit<N>, hipFuncAttributeMaxDynamicSharedMemorySize, FitWords<N>::TOTAL * 64 * 8);
    if (e != hipSuccess) return e;
    const int groups = 64 >> lg;
    const size_t lds = (size_t)FitWords<N>::TOTAL * groups * sizeof(double);
    hipLaunchKernelGGL(k_fit<N>, dim3((unsigned)((n_jobs + groups - 1) / groups)), dim3(64), lds, s, jobs, n_jobs, lg, points, prad, centers, radii);
    return hipGetLastError();
}

int fit_spheres_device(ndt_hip_ctx *ctx, int dims, long long n_lists, const int64_t *first, const double *points, const double *point_radius,
                       double *centers, double *radii)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const long long n_points = first[n_lists];
    // lists by lanes per fit, then by length (neighbouring lanes walk lists of equal length), then by position
    std::vector<FitJob> jobs((size_t)n_lists);
    for (long long i = 0; i < n_lists; ++i) jobs[(size_t)i] = { first[i], (int)(first[i + 1] - first[i]), (int)i };
    std::sort(jobs.begin(), jobs.end(), [](const FitJob &a, const FitJob &b) { return a.count != b.count ? a.count < b.count : a.list < b.list; });

    // one grow-only device buffer of the context: jobs | points | point radii | centres | radii
    const size_t o_jobs = 0, o_pts = o_jobs + sizeof(FitJob) * (size_t)n_lists, o_rad = o_pts + sizeof(double) * (size_t)n_points * dims,
                 o_cen = o_rad + sizeof(double) * (size_t)n_points, o_out = o_cen + sizeof(double) * (size_t)n_lists * dims,
                 total = o_out + sizeof(double) * (size_t)n_lists;
    const int rc = ctx->d_fit.reserve(total, ctx->stream, "ndt_hip_fit_spheres", true);      // head room: frame-to-frame counts vary
    if (rc) return rc;
    char *base = ctx->d_fit.as<char>();
    hipStream_t s = ctx->stream;
    HIP_TRY(hipMemcpyAsync(base + o_jobs, jobs.data(), sizeof(FitJob) * (size_t)n_lists, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + o_pts, points, sizeof(double) * (size_t)n_points * dims, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + o_rad, point_radius, sizeof(double) * (size_t)n_points, hipMemcpyHostToDevice, s));
    int n_launch = 0;
    for (size_t b = 0; b < jobs.size();) {
        const int lg = fit_lg_lanes(jobs[b].count);
        size_t e = b;
        while (e < jobs.size() && fit_lg_lanes(jobs[e].count) == lg) ++e;
        const FitJob *dj = (const FitJob *)(base + o_jobs) + b;
        const double *dp = (const double *)(base + o_pts), *dr = (const double *)(base + o_rad);
        double *dc = (double *)(base + o_cen), *dq = (double *)(base + o_out);
        const int n = (int)(e - b);
        hipError_t err = hipSuccess;
        switch (dims) {
        case 3: err = launch_fit<3>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 4: err = launch_fit<4>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 5: err = launch_fit<5>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 6: err = launch_fit<6>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 7: err = launch_fit<7>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 8: err = launch_fit<8>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 9: err = launch_fit<9>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 10: err = launch_fit<10>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 11: err = launch_fit<11>(s, dj, n, lg, dp, dr, dc, dq); break;
        case 12: err = launch_fit<12>(s, dj, n, lg, dp, dr, dc, dq); break;
        default: return fail(NDT_E_INVALID, "%d dimensions", dims);
        }
        if (err != hipSuccess) return fail(NDT_E_DEVICE, "fit kernel (%d-D, %d lanes a fit): %s", dims, 1 << lg, hipGetErrorString(err));
        ++n_launch;
        b = e;
    }
    HIP_TRY(hipMemcpyAsync(centers, base + o_cen, sizeof(double) * (size_t)n_lists * dims, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(radii, base + o_out, sizeof(double) * (size_t)n_lists, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ctx->fit_launches = n_launch;
    return NDT_OK;
}

} // namespace ndt_impl
