// ndt_denoise.hip -- a sampled frame denoised on the device (`ndt_hip --denoise`): an edge-avoiding a-trous wavelet over the double
// framebuffer, in linear light, before pixel_d2c, guided by what ndt_hip_render_features knows of every pixel -- the object its
// primary ray hits, the N-D hit point and the N-D normal there.  ndt_hip_denoise_device / ndt_hip_render_denoised*.
//
// Iteration it = 0 .. iterations - 1 has step s = 1 << it and reads image `cur`, writes `next`.  A pixel p whose id is 0 is copied.
// Every other pixel is the weighted mean of the 5 x 5 taps q = p + (j - 2, i - 2) * s (j outer, i inner) of the B3 spline
// H = {1/16, 1/4, 3/8, 1/4, 1/16}: the centre with weight h = H[j] H[i], always; any other tap only inside the image (no wrap, no
// clamp), only on the same object, and with
//     w = ((h * wn) * wp) * wc      wn = max(n_p . n_q, 0) squared normal_power_log2 times
//                                   wp = 1 - ((n_p . d)^2 / (d . d)) / sigma_plane^2,  d = P_q - P_p (1 where d . d is not > 0)
//                                   wc = 1 / (1 + |rgb_q - rgb_p|^2 / (sigma_colour / s)^2)
// when w > 0 (a NaN is dropped with that).  Sums run over components in ascending order, one operation at a time; include/ndt_hip.h
// has the definition to the bit, and under -ffp-contract=off a numpy restatement gives the same 64-bit patterns.
//
//   k_denoise_atrous<N>   one launch an iteration, one lane a pixel, consecutive lanes on consecutive pixels: every plane load and
//                         every 32-byte colour load is contiguous across the wavefront at any step.  The centre's normal and
//                         position stay in registers; a tap's guide planes are not loaded when its id differs or it lies outside.
// No atomics, no LDS, no workgroup waits for another, trip counts come from sizes.  The iterations ping-pong between two buffers of
// the context; the last one writes the destination.
#include "ndt_ctx.hpp"
#include <limits.h>

namespace {

constexpr int DENOISE_LANES = 256;
constexpr int FEATURES_ALL = NDT_FEATURE_ID | NDT_FEATURE_POSITION | NDT_FEATURE_NORMAL;

template <int N>
__global__ void __launch_bounds__(DENOISE_LANES) k_denoise_atrous(const double2 *__restrict__ cur, double2 *__restrict__ next,
                                                                  const int *__restrict__ id, const double *__restrict__ position,
                                                                  const double *__restrict__ normal, int width, int rows, int step,
                                                                  double inv_c, double inv_p, int normal_power_log2)
{
    const long long n_pixels = (long long)rows * width;
    const long long p = (long long)blockIdx.x * DENOISE_LANES + threadIdx.x;
    if (p >= n_pixels) return;
    const int y = (int)(p / width), x = (int)(p - (long long)y * width);
    const double2 p_rg = cur[2 * p], p_ba = cur[2 * p + 1];
    const int me = id[p];
    if (me == 0) {
        next[2 * p] = p_rg;
        next[2 * p + 1] = p_ba;
        return;
    }
    double pn[N], pp[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        pn[k] = normal[(long long)k * n_pixels + p];
        pp[k] = position[(long long)k * n_pixels + p];
    }
    double num0 = 0.0, num1 = 0.0, num2 = 0.0, num3 = 0.0, den = 0.0;
#pragma unroll 1
    for (int j = 0; j < 5; ++j) {
        const double hj = j == 2 ? 0.375 : (j == 1 || j == 3) ? 0.25 : 0.0625;
        const int qy = y + (j - 2) * step;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double h = hj * (i == 2 ? 0.375 : (i == 1 || i == 3) ? 0.25 : 0.0625);
            const int qx = x + (i - 2) * step;
            double w = h;
            double2 q_rg = p_rg, q_ba = p_ba;
            if (j != 2 || i != 2) {
                if (qy < 0 || qy >= rows || qx < 0 || qx >= width) continue;
                const long long q = (long long)qy * width + qx;
                if (id[q] != me) continue;
                double dd = 0.0, nd = 0.0, dot = 0.0;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double d = position[(long long)k * n_pixels + q] - pp[k];
                    dd = dd + d * d;
                    nd = nd + pn[k] * d;
                    dot = dot + pn[k] * normal[(long long)k * n_pixels + q];
                }
                double wn = dot > 0 ? dot : 0;
                for (int e = 0; e < normal_power_log2; ++e) wn = wn * wn;
                const double wp = dd > 0 ? 1.0 - ((nd * nd) / dd) * inv_p : 1.0;
                q_rg = cur[2 * q];
                q_ba = cur[2 * q + 1];
                const double dr = q_rg.x - p_rg.x, dg = q_rg.y - p_rg.y, db = q_ba.x - p_ba.x;
                const double cc = (dr * dr + dg * dg) + db * db;
                const double wc = 1.0 / (1.0 + cc * inv_c);
                w = ((h * wn) * wp) * wc;
                if (!(w > 0)) continue;
            }
            num0 = num0 + w * q_rg.x;
            num1 = num1 + w * q_rg.y;
            num2 = num2 + w * q_ba.x;
            num3 = num3 + w * q_ba.y;
            den = den + w;
        }
    }
    next[2 * p] = make_double2(num0 / den, num1 / den);
    next[2 * p + 1] = make_double2(num2 / den, num3 / den);
}

template <int N>
void launch_atrous(hipStream_t s, unsigned grid, const void *cur, void *next, const ndt_feature_planes &g, int width, int rows, int step,
                   double inv_c, double inv_p, int normal_power_log2)
{
    hipLaunchKernelGGL(k_denoise_atrous<N>, dim3(grid), dim3(DENOISE_LANES), 0, s, (const double2 *)cur, (double2 *)next, (const int *)g.id,
                       (const double *)g.position, (const double *)g.normal, width, rows, step, inv_c, inv_p, normal_power_log2);
}

// The variance-guided filter (`ndt_hip --vdenoise`; include/ndt_hip.h has the definition to the bit): the same taps, guides and
// launch shape, but the colour weight's width comes from the frame -- sp = k_colour^2 times the 3 x 3 binomial mean, over the
// pixel's own object, of the variance plane at distance 1 -- and the plane is carried along: vnext = sum w^2 vcur / (sum w)^2.
// A pixel without variance (!(sp > 0): it has converged, or its plane holds a NaN) is copied bit for bit, as the background is.
//   k_sample_variance     the plane of a frame from its sample moments (ndt_hip_render_moments*): one lane a pixel
//   k_vdenoise_atrous<N>  one launch an iteration, one lane a pixel; reads (cur, vcur), writes (next, vnext)
__global__ void __launch_bounds__(DENOISE_LANES) k_sample_variance(const double *__restrict__ rgba, const int *__restrict__ count,
                                                                   const double *__restrict__ sum_sq, double *__restrict__ variance, long long n_pixels)
{
    const long long p = (long long)blockIdx.x * DENOISE_LANES + threadIdx.x;
    if (p >= n_pixels) return;
    const int n = count[p];
    double v = 0.0;
    if (n >= 2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double m = rgba[4 * p + c];
            double e = sum_sq[(long long)c * n_pixels + p] / (double)n - m * m;
            e = e > 0 ? e : 0.0;
            v = v + e / (double)(n - 1);
        }
    }
    variance[p] = v;
}

template <int N>
__global__ void __launch_bounds__(DENOISE_LANES) k_vdenoise_atrous(const double2 *__restrict__ cur, double2 *__restrict__ next,
                                                                   const double *__restrict__ vcur, double *__restrict__ vnext,
                                                                   const int *__restrict__ id, const double *__restrict__ position,
                                                                   const double *__restrict__ normal, int width, int rows, int step,
                                                                   double k2, double inv_p, int normal_power_log2)
{
    const long long n_pixels = (long long)rows * width;
    const long long p = (long long)blockIdx.x * DENOISE_LANES + threadIdx.x;
    if (p >= n_pixels) return;
    const int y = (int)(p / width), x = (int)(p - (long long)y * width);
    const double2 p_rg = cur[2 * p], p_ba = cur[2 * p + 1];
    const double p_v = vcur[p];
    const int me = id[p];
    double sp = 0.0;
    if (me != 0) {
        // the local variance: always at distance 1, whatever the step
        double gn = 0.0, gd = 0.0;
#pragma unroll 1
        for (int b = 0; b < 3; ++b) {
            const double gb = b == 1 ? 0.5 : 0.25;
            const int ry = y + b - 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double g = gb * (a == 1 ? 0.5 : 0.25);
                const int rx = x + a - 1;
                if (ry < 0 || ry >= rows || rx < 0 || rx >= width) continue;
                const long long r = (long long)ry * width + rx;
                if (id[r] != me) continue;
                gn = gn + g * vcur[r];
                gd = gd + g;
            }
        }
        sp = k2 * (gn / gd);
    }
    if (!(sp > 0)) {        // (the background too: its sp is 0)
        next[2 * p] = p_rg;
        next[2 * p + 1] = p_ba;
        vnext[p] = p_v;
        return;
    }
    double pn[N], pp[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        pn[k] = normal[(long long)k * n_pixels + p];
        pp[k] = position[(long long)k * n_pixels + p];
    }
    double num0 = 0.0, num1 = 0.0, num2 = 0.0, num3 = 0.0, den = 0.0, vn = 0.0;
#pragma unroll 1
    for (int j = 0; j < 5; ++j) {
        const double hj = j == 2 ? 0.375 : (j == 1 || j == 3) ? 0.25 : 0.0625;
        const int qy = y + (j - 2) * step;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double h = hj * (i == 2 ? 0.375 : (i == 1 || i == 3) ? 0.25 : 0.0625);
            const int qx = x + (i - 2) * step;
            double w = h, q_v = p_v;
            double2 q_rg = p_rg, q_ba = p_ba;
            if (j != 2 || i != 2) {
                if (qy < 0 || qy >= rows || qx < 0 || qx >= width) continue;
                const long long q = (long long)qy * width + qx;
                if (id[q] != me) continue;
                double dd = 0.0, nd = 0.0, dot = 0.0;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double d = position[(long long)k * n_pixels + q] - pp[k];
                    dd = dd + d * d;
                    nd = nd + pn[k] * d;
                    dot = dot + pn[k] * normal[(long long)k * n_pixels + q];
                }
                double wn = dot > 0 ? dot : 0;
                for (int e = 0; e < normal_power_log2; ++e) wn = wn * wn;
                const double wp = dd > 0 ? 1.0 - ((nd * nd) / dd) * inv_p : 1.0;
                q_rg = cur[2 * q];
                q_ba = cur[2 * q + 1];
                const double dr = q_rg.x - p_rg.x, dg = q_rg.y - p_rg.y, db = q_ba.x - p_ba.x;
                const double cc = (dr * dr + dg * dg) + db * db;
                const double wc = 1.0 / (1.0 + cc / sp);
                w = ((h * wn) * wp) * wc;
                if (!(w > 0)) continue;
                q_v = vcur[q];
            }
            num0 = num0 + w * q_rg.x;
            num1 = num1 + w * q_rg.y;
            num2 = num2 + w * q_ba.x;
            num3 = num3 + w * q_ba.y;
            den = den + w;
            vn = vn + (w * w) * q_v;
        }
    }
    next[2 * p] = make_double2(num0 / den, num1 / den);
    next[2 * p + 1] = make_double2(num2 / den, num3 / den);
    vnext[p] = vn / (den * den);
}

template <int N>
void launch_vatrous(hipStream_t s, unsigned grid, const void *cur, void *next, const void *vcur, void *vnext, const ndt_feature_planes &g,
                    int width, int rows, int step, double k2, double inv_p, int normal_power_log2)
{
    hipLaunchKernelGGL(k_vdenoise_atrous<N>, dim3(grid), dim3(DENOISE_LANES), 0, s, (const double2 *)cur, (double2 *)next, (const double *)vcur,
                       (double *)vnext, (const int *)g.id, (const double *)g.position, (const double *)g.normal, width, rows, step, k2, inv_p,
                       normal_power_log2);
}

ndt_vdenoise_params vparams_of(const ndt_vdenoise_params *vp)
{
    if (vp) return *vp;
    ndt_vdenoise_params d;
    d.iterations = 4;
    d.normal_power_log2 = 5;
    d.k_colour = 4.0;
    d.sigma_plane = 0.25;
    return d;
}

int check_vparams(const char *who, const ndt_vdenoise_params &d)
{
    if (d.iterations < 1 || d.iterations > 6) return fail(NDT_E_INVALID, "%s: %d iterations are outside 1 .. 6", who, d.iterations);
    if (d.normal_power_log2 < 0 || d.normal_power_log2 > 8)
        return fail(NDT_E_INVALID, "%s: normal_power_log2 %d is outside 0 .. 8", who, d.normal_power_log2);
    if (!(d.k_colour > 0) || !isfinite(d.k_colour)) return fail(NDT_E_INVALID, "%s: k_colour %g: a finite number above 0", who, d.k_colour);
    if (!(d.sigma_plane > 0) || !isfinite(d.sigma_plane)) return fail(NDT_E_INVALID, "%s: sigma_plane %g: a finite number above 0", who, d.sigma_plane);
    return NDT_OK;
}

ndt_denoise_params params_of(const ndt_denoise_params *dp)
{
    if (dp) return *dp;
    ndt_denoise_params d;
    d.iterations = 4;
    d.normal_power_log2 = 5;
    d.sigma_colour = 0.25;
    d.sigma_plane = 0.25;
    return d;
}

int check_params(const char *who, const ndt_denoise_params &d)
{
    if (d.iterations < 1 || d.iterations > 6) return fail(NDT_E_INVALID, "%s: %d iterations are outside 1 .. 6", who, d.iterations);
    if (d.normal_power_log2 < 0 || d.normal_power_log2 > 8)
        return fail(NDT_E_INVALID, "%s: normal_power_log2 %d is outside 0 .. 8", who, d.normal_power_log2);
    if (!(d.sigma_colour > 0) || !isfinite(d.sigma_colour))
        return fail(NDT_E_INVALID, "%s: sigma_colour %g: a finite number above 0", who, d.sigma_colour);
    if (!(d.sigma_plane > 0) || !isfinite(d.sigma_plane)) return fail(NDT_E_INVALID, "%s: sigma_plane %g: a finite number above 0", who, d.sigma_plane);
    return NDT_OK;
}

// The iterations for checked arguments, asynchronous on the context's stream: d_in -> ping -> pong -> ... -> d_out.  d_out may be
// d_in: a single iteration then goes through ping and a copy.
int iterate(ndt_hip_ctx *ctx, const char *who, const void *d_in, const ndt_feature_planes &g, int dims, int width, int rows,
            const ndt_denoise_params &d, void *d_out)
{
    DenoiseState &dn = ctx->denoise;
    hipStream_t s = ctx->stream;
    const long long n_pixels = (long long)rows * width;
    const long long grid = (n_pixels + DENOISE_LANES - 1) / DENOISE_LANES;
    if (grid > INT_MAX) return fail(NDT_E_UNSUPPORTED, "%s: %d x %d pixels are more than one launch takes", who, width, rows);
    const size_t img_bytes = (size_t)n_pixels * 4 * sizeof(double);
    const bool through_copy = d.iterations == 1 && d_in == d_out;
    int rc;
    if ((d.iterations > 1 || through_copy) && (rc = dn.d_ping.reserve(img_bytes, s, who))) return rc;
    if (d.iterations > 2 && (rc = dn.d_pong.reserve(img_bytes, s, who))) return rc;
    if (!dn.ev[0])
        for (hipEvent_t &e : dn.ev) HIP_TRY(hipEventCreate(&e));
    const double inv_p = 1.0 / (d.sigma_plane * d.sigma_plane);
    const void *cur = d_in;
    for (int it = 0; it < d.iterations; ++it) {
        const bool last = it == d.iterations - 1;
        void *next = last && !through_copy ? d_out : (it & 1) ? dn.d_pong.p : dn.d_ping.p;
        const double sc = d.sigma_colour / (double)(1 << it);
        const double inv_c = 1.0 / (sc * sc);
        const int step = 1 << it;
        HIP_TRY(hipEventRecord(dn.ev[2 * it], s));
        switch (dims) {
        case 3: launch_atrous<3>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        case 4: launch_atrous<4>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        case 5: launch_atrous<5>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        case 6: launch_atrous<6>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        case 7: launch_atrous<7>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        case 8: launch_atrous<8>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        case 9: launch_atrous<9>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        case 10: launch_atrous<10>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        case 11: launch_atrous<11>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        default: launch_atrous<12>(s, (unsigned)grid, cur, next, g, width, rows, step, inv_c, inv_p, d.normal_power_log2); break;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(dn.ev[2 * it + 1], s));
        ++dn.launches;
        cur = next;
    }
    if (through_copy) HIP_TRY(hipMemcpyAsync(d_out, dn.d_ping.p, img_bytes, hipMemcpyDeviceToDevice, s));
    dn.iterations = d.iterations;
    return NDT_OK;
}

// The variance-guided iterations for checked arguments, asynchronous on the context's stream: (d_in, d_var) -> (ping, vping) ->
// (pong, vpong) -> ... -> (d_out, d_var_out).  d_out may be d_in and d_var_out d_var: a single iteration then goes through the
// context's buffer and a copy.  d_var_out nullptr: the last plane stays in the context's buffer.
int viterate(ndt_hip_ctx *ctx, const char *who, const void *d_in, const void *d_var, const ndt_feature_planes &g, int dims, int width, int rows,
             const ndt_vdenoise_params &d, void *d_out, void *d_var_out)
{
    DenoiseState &dn = ctx->denoise;
    hipStream_t s = ctx->stream;
    const long long n_pixels = (long long)rows * width;
    const long long grid = (n_pixels + DENOISE_LANES - 1) / DENOISE_LANES;
    if (grid > INT_MAX) return fail(NDT_E_UNSUPPORTED, "%s: %d x %d pixels are more than one launch takes", who, width, rows);
    const size_t img_bytes = (size_t)n_pixels * 4 * sizeof(double), var_bytes = (size_t)n_pixels * sizeof(double);
    const bool through_copy = d.iterations == 1 && d_in == d_out, v_through_copy = d.iterations == 1 && d_var == d_var_out;
    int rc;
    if ((d.iterations > 1 || through_copy) && (rc = dn.d_ping.reserve(img_bytes, s, who))) return rc;
    if (d.iterations > 2 && (rc = dn.d_pong.reserve(img_bytes, s, who))) return rc;
    if ((rc = dn.d_vping.reserve(var_bytes, s, who))) return rc;
    if (d.iterations > 1 && (rc = dn.d_vpong.reserve(var_bytes, s, who))) return rc;
    if (!dn.ev[0])
        for (hipEvent_t &e : dn.ev) HIP_TRY(hipEventCreate(&e));
    const double inv_p = 1.0 / (d.sigma_plane * d.sigma_plane), k2 = d.k_colour * d.k_colour;
    const void *cur = d_in, *vcur = d_var;
    for (int it = 0; it < d.iterations; ++it) {
        const bool last = it == d.iterations - 1;
        void *next = last && !through_copy ? d_out : (it & 1) ? dn.d_pong.p : dn.d_ping.p;
        void *vnext = last && d_var_out && !v_through_copy ? d_var_out : (it & 1) ? dn.d_vpong.p : dn.d_vping.p;
        const int step = 1 << it;
        HIP_TRY(hipEventRecord(dn.ev[2 * it], s));
        switch (dims) {
        case 3: launch_vatrous<3>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        case 4: launch_vatrous<4>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        case 5: launch_vatrous<5>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        case 6: launch_vatrous<6>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        case 7: launch_vatrous<7>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        case 8: launch_vatrous<8>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        case 9: launch_vatrous<9>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        case 10: launch_vatrous<10>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        case 11: launch_vatrous<11>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        default: launch_vatrous<12>(s, (unsigned)grid, cur, next, vcur, vnext, g, width, rows, step, k2, inv_p, d.normal_power_log2); break;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(dn.ev[2 * it + 1], s));
        ++dn.launches;
        cur = next;
        vcur = vnext;
    }
    if (through_copy) HIP_TRY(hipMemcpyAsync(d_out, dn.d_ping.p, img_bytes, hipMemcpyDeviceToDevice, s));
    if (v_through_copy) HIP_TRY(hipMemcpyAsync(d_var_out, dn.d_vping.p, var_bytes, hipMemcpyDeviceToDevice, s));
    dn.iterations = d.iterations;
    return NDT_OK;
}

// after the stream has been synchronised: the summed device time of the last call's iterations
int collect_ms(ndt_hip_ctx *ctx)
{
    DenoiseState &dn = ctx->denoise;
    dn.ms = 0.0;
    for (int it = 0; it < dn.iterations; ++it) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, dn.ev[2 * it], dn.ev[2 * it + 1]));
        dn.ms += ms;
    }
    return NDT_OK;
}

int refuse_frame(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, FrameView *v);

// what every whole-frame call refuses, before any device work; *d the parameters in force, *v the frame's width and rows
// (refuse_frame: the frames, whichever filter)
int refuse(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, const void *out, ndt_denoise_params *d,
           FrameView *v)
{
    if (!ctx || !p || !out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    *v = FrameView{ nullptr, nullptr, nullptr, p->width, 0 };
    *d = params_of(dp);
    const int rc = check_params(who, *d);
    return rc ? rc : refuse_frame(who, ctx, p, v);
}

// ... and of the variance-guided filter: the same, plus what the sample moments refuse
int vrefuse(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, const void *out, ndt_vdenoise_params *d,
            FrameView *v)
{
    if (!ctx || !p || !out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    *v = FrameView{ nullptr, nullptr, nullptr, p->width, 0 };
    *d = vparams_of(vp);
    int rc = check_vparams(who, *d);
    if (rc) return rc;
    if ((rc = refuse_frame(who, ctx, p, v))) return rc;
    return moments_refuse(who, p);
}

int refuse_frame(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, FrameView *v)
{
    if (p->recursive_aa)
        return fail(NDT_E_UNSUPPORTED, "%s: no denoiser behind recursive_aa (-a): its pixels are averages of corner samples, the guides are one ray's", who);
    if (p->stereo != NDT_STEREO_MONO)
        return fail(NDT_E_UNSUPPORTED, "%s: no denoiser for stereo mode %d: a stencil must not cross the seam between two eyes", who, p->stereo);
    if (p->row_begin != 0 || p->row_step != 1)
        return fail(NDT_E_UNSUPPORTED, "%s: no denoiser for a row shard (row_begin %d, row_step %d): a cyclic shard has no neighbouring rows", who,
                    p->row_begin, p->row_step);
    if (p->samples < 1) return fail(NDT_E_INVALID, "%s: samples=%d", who, p->samples);
    ndt_render_params q = *p;
    q.samples = 1;
    return features_check(who, ctx, &q, &v->rows);
}

// The denoised frame of checked arguments in d_rgba (device, aligned to 16 bytes): the frame `p` asks for into the context's frame
// buffer, the feature pass of the same frame with samples = 1 into the context's planes, the iterations.  Returns when complete.
int render_denoised(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params &d, int rows, void *d_rgba,
                    ndt_render_stats *stats)
{
    HIP_TRY(hipSetDevice(ctx->device));
    DenoiseState &dn = ctx->denoise;
    dn.launches = 0;
    dn.iterations = 0;
    dn.ms = 0.0;
    const size_t img_bytes = (size_t)rows * (size_t)p->width * 4 * sizeof(double);
    int rc;
    if ((rc = dn.d_frame.reserve(img_bytes, ctx->stream, who))) return rc;
    if ((rc = ndt_hip_render_device(ctx, p, dn.d_frame.p, stats))) return rc;
    ndt_render_params q = *p;
    q.samples = 1;
    ndt_feature_planes planes;
    if ((rc = features_own(ctx, who, &q, FEATURES_ALL, false, &planes))) return rc;
    dn.launches = ctx->features.launches;
    if ((rc = iterate(ctx, who, dn.d_frame.p, planes, ctx->dims, p->width, rows, d, d_rgba))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return collect_ms(ctx);
}

// ... into the context's own buffer dn.d_out (*v: sized by refuse)
int render_denoised_own(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params &d, ndt_render_stats *stats, FrameView *v)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = ctx->denoise.d_out.reserve(v->pixels() * 4 * sizeof(double), ctx->stream, who);
    if (rc) return rc;
    v->d_rgba = ctx->denoise.d_out.p;
    return render_denoised(who, ctx, p, d, v->rows, ctx->denoise.d_out.p, stats);
}

// The variance-guided frame of checked arguments in d_rgba (device, aligned to 16 bytes): the frame `p` asks for and its sample
// moments into the context's buffers, the feature pass of the same frame with samples = 1, the variance plane of the moments, the
// iterations.  Returns when complete.
int render_vdenoised(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params &d, int rows, void *d_rgba,
                     ndt_render_stats *stats)
{
    HIP_TRY(hipSetDevice(ctx->device));
    DenoiseState &dn = ctx->denoise;
    dn.launches = 0;
    dn.iterations = 0;
    dn.ms = 0.0;
    const size_t pixels = (size_t)rows * (size_t)p->width;
    int rc;
    if ((rc = dn.d_frame.reserve(pixels * 4 * sizeof(double), ctx->stream, who))) return rc;
    if ((rc = dn.d_moments.reserve(pixels * (3 * sizeof(double) + sizeof(int32_t)), ctx->stream, who))) return rc;
    if ((rc = dn.d_variance.reserve(pixels * sizeof(double), ctx->stream, who))) return rc;
    void *d_sum_sq = dn.d_moments.p, *d_count = dn.d_moments.as<char>() + pixels * 3 * sizeof(double);
    if ((rc = ndt_hip_render_moments_device(ctx, p, dn.d_frame.p, d_count, d_sum_sq, stats))) return rc;
    ndt_render_params q = *p;
    q.samples = 1;
    ndt_feature_planes planes;
    if ((rc = features_own(ctx, who, &q, FEATURES_ALL, false, &planes))) return rc;
    hipLaunchKernelGGL(k_sample_variance, dim3((unsigned)((pixels + DENOISE_LANES - 1) / DENOISE_LANES)), dim3(DENOISE_LANES), 0, ctx->stream,
                       dn.d_frame.as<double>(), (const int *)d_count, (const double *)d_sum_sq, dn.d_variance.as<double>(), (long long)pixels);
    HIP_TRY(hipGetLastError());
    dn.launches = ctx->features.launches + 1;
    if ((rc = viterate(ctx, who, dn.d_frame.p, dn.d_variance.p, planes, ctx->dims, p->width, rows, d, d_rgba, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return collect_ms(ctx);
}

// ... into the context's own buffer dn.d_out (*v: sized by vrefuse)
int render_vdenoised_own(const char *who, ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params &d, ndt_render_stats *stats, FrameView *v)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = ctx->denoise.d_out.reserve(v->pixels() * 4 * sizeof(double), ctx->stream, who);
    if (rc) return rc;
    v->d_rgba = ctx->denoise.d_out.p;
    return render_vdenoised(who, ctx, p, d, v->rows, ctx->denoise.d_out.p, stats);
}

} // namespace

void ndt_impl::free_denoise(ndt_hip_ctx *ctx)
{
    DenoiseState &dn = ctx->denoise;
    dn.d_ping.release();
    dn.d_pong.release();
    dn.d_vping.release();
    dn.d_vpong.release();
    dn.d_moments.release();
    dn.d_variance.release();
    dn.d_frame.release();
    dn.d_out.release();
    dn.d_rgba8.release();
    for (hipEvent_t &e : dn.ev)
        if (e) (void)hipEventDestroy(e);
    dn = DenoiseState();
}

extern "C" int ndt_hip_denoise_device(ndt_hip_ctx *ctx, const void *d_rgba_in, const ndt_feature_planes *d_planes, int32_t dims, int32_t width,
                                      int32_t rows, const ndt_denoise_params *dp, void *d_rgba_out)
{
    const char *who = "ndt_hip_denoise_device";
    if (!ctx || !d_rgba_in || !d_planes || !d_rgba_out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    const ndt_denoise_params d = params_of(dp);
    int rc = check_params(who, d);
    if (rc) return rc;
    if (dims < NDT_MIN_DIMS || dims > NDT_MAX_DIMS) return fail(NDT_E_INVALID, "%s: %d dimensions are outside %d .. %d", who, dims, NDT_MIN_DIMS, NDT_MAX_DIMS);
    if (width < 1 || rows < 1) return fail(NDT_E_INVALID, "%s: a frame of %d x %d pixels", who, width, rows);
    if (!d_planes->id || !d_planes->position || !d_planes->normal)
        return fail(NDT_E_INVALID, "%s: a NULL plane: id, position and normal guide the filter", who);
    if (((uintptr_t)d_rgba_in & 15u) != 0 || ((uintptr_t)d_rgba_out & 15u) != 0 || ((uintptr_t)d_planes->id & 3u) != 0 ||
        (((uintptr_t)d_planes->position | (uintptr_t)d_planes->normal) & 7u) != 0)
        return fail(NDT_E_INVALID, "%s: misaligned: the images to 16 bytes, the planes to their elements", who);
    HIP_TRY(hipSetDevice(ctx->device));
    DenoiseState &dn = ctx->denoise;
    dn.launches = 0;
    dn.iterations = 0;
    dn.ms = 0.0;
    if ((rc = iterate(ctx, who, d_rgba_in, *d_planes, dims, width, rows, d, d_rgba_out))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return collect_ms(ctx);
}

extern "C" int ndt_hip_denoise_launches(ndt_hip_ctx *ctx) { return ctx ? ctx->denoise.launches : 0; }
extern "C" double ndt_hip_denoise_ms(ndt_hip_ctx *ctx) { return ctx ? ctx->denoise.ms : 0.0; }

extern "C" int ndt_hip_render_denoised_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, void *d_rgba,
                                              ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_denoised_device";
    ndt_denoise_params d;
    FrameView v;
    int rc = refuse(who, ctx, p, dp, d_rgba, &d, &v);
    if (rc) return rc;
    if (((uintptr_t)d_rgba & 15u) != 0) return fail(NDT_E_INVALID, "%s: misaligned: the image must be aligned to 16 bytes", who);
    return render_denoised(who, ctx, p, d, v.rows, d_rgba, stats);
}

// The delivering entries (the 8-bit image of those that want one: quantised into dn.d_rgba8 by the tail)
extern "C" int ndt_hip_render_denoised(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, double *rgba,
                                       ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_denoised";
    ndt_denoise_params d;
    FrameView v;
    int rc = refuse(who, ctx, p, dp, rgba, &d, &v);
    if (rc) return rc;
    if ((rc = render_denoised_own(who, ctx, p, d, stats, &v))) return rc;
    return deliver_doubles(ctx, v, rgba, nullptr);
}

extern "C" int ndt_hip_render_denoised_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, uint8_t *rgba8,
                                             ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_denoised_rgba8";
    ndt_denoise_params d;
    FrameView v;
    int rc = refuse(who, ctx, p, dp, rgba8, &d, &v);
    if (rc) return rc;
    if ((rc = render_denoised_own(who, ctx, p, d, stats, &v))) return rc;
    return deliver_rgba8(ctx, who, v, ctx->denoise.d_rgba8, rgba8);
}

extern "C" int ndt_hip_render_denoised_png(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, uint8_t *png, int64_t cap,
                                           ndt_png_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_denoised_png";
    ndt_denoise_params d;
    FrameView v;
    int rc = refuse(who, ctx, p, dp, png, &d, &v);
    if (rc) return rc;
    if ((rc = refuse_png(who, p->width, v.rows, 4))) return rc;
    if ((rc = render_denoised_own(who, ctx, p, d, render_stats, &v))) return rc;
    return deliver_png(ctx, who, v, ctx->denoise.d_rgba8, png, cap, stats);
}

extern "C" int ndt_hip_render_denoised_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, const ndt_jpeg_params *jp,
                                            uint8_t *jpg, int64_t cap, ndt_jpeg_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_denoised_jpeg";
    ndt_denoise_params d;
    FrameView v;
    int rc = refuse(who, ctx, p, dp, jpg, &d, &v);
    if (rc) return rc;
    if ((rc = refuse_jpeg(who, p->width, v.rows, jp))) return rc;
    if ((rc = render_denoised_own(who, ctx, p, d, render_stats, &v))) return rc;
    return deliver_jpeg(ctx, who, v, ctx->denoise.d_rgba8, jp, jpg, cap, stats);
}

extern "C" int ndt_hip_render_denoised_exr(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_denoise_params *dp, const ndt_exr_params *ep,
                                           uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_denoised_exr";
    if (stats) *stats = ndt_exr_stats{};
    ndt_denoise_params d;
    FrameView v;
    int rc = refuse(who, ctx, p, dp, out, &d, &v);
    if (rc) return rc;
    if (ndt_hip_exr_bound(p->width, v.rows, ep, 0) < 0)
        return fail(NDT_E_INVALID, "%s: no EXR of %d x %d with these parameters (a pixel type other than 0, 1, 2, or samples beyond 2^31 - 1 bytes)", who,
                    p->width, v.rows);
    if ((rc = render_denoised_own(who, ctx, p, d, render_stats, &v))) return rc;
    return deliver_exr(ctx, v, ep, out, cap, stats);
}

// ---------------------------------------------------------------- the variance-guided filter's entries

extern "C" int ndt_hip_sample_variance_device(ndt_hip_ctx *ctx, const void *d_rgba, const void *d_count, const void *d_sum_sq, int32_t width,
                                              int32_t rows, void *d_variance)
{
    const char *who = "ndt_hip_sample_variance_device";
    if (!ctx || !d_rgba || !d_count || !d_sum_sq || !d_variance) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    if (width < 1 || rows < 1) return fail(NDT_E_INVALID, "%s: a frame of %d x %d pixels", who, width, rows);
    if ((((uintptr_t)d_rgba | (uintptr_t)d_sum_sq | (uintptr_t)d_variance) & 7u) != 0 || ((uintptr_t)d_count & 3u) != 0)
        return fail(NDT_E_INVALID, "%s: misaligned: the doubles to 8 bytes, the counts to 4", who);
    const long long n_pixels = (long long)rows * width;
    const long long grid = (n_pixels + DENOISE_LANES - 1) / DENOISE_LANES;
    if (grid > INT_MAX) return fail(NDT_E_UNSUPPORTED, "%s: %d x %d pixels are more than one launch takes", who, width, rows);
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_sample_variance, dim3((unsigned)grid), dim3(DENOISE_LANES), 0, ctx->stream, (const double *)d_rgba, (const int *)d_count,
                       (const double *)d_sum_sq, (double *)d_variance, n_pixels);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return NDT_OK;
}

extern "C" int ndt_hip_vdenoise_device(ndt_hip_ctx *ctx, const void *d_rgba_in, const ndt_feature_planes *d_planes, const void *d_variance,
                                       int32_t dims, int32_t width, int32_t rows, const ndt_vdenoise_params *vp, void *d_rgba_out,
                                       void *d_variance_out)
{
    const char *who = "ndt_hip_vdenoise_device";
    if (!ctx || !d_rgba_in || !d_planes || !d_variance || !d_rgba_out) return fail(NDT_E_INVALID, "%s: NULL argument", who);
    const ndt_vdenoise_params d = vparams_of(vp);
    int rc = check_vparams(who, d);
    if (rc) return rc;
    if (dims < NDT_MIN_DIMS || dims > NDT_MAX_DIMS) return fail(NDT_E_INVALID, "%s: %d dimensions are outside %d .. %d", who, dims, NDT_MIN_DIMS, NDT_MAX_DIMS);
    if (width < 1 || rows < 1) return fail(NDT_E_INVALID, "%s: a frame of %d x %d pixels", who, width, rows);
    if (!d_planes->id || !d_planes->position || !d_planes->normal)
        return fail(NDT_E_INVALID, "%s: a NULL plane: id, position and normal guide the filter", who);
    if (((uintptr_t)d_rgba_in & 15u) != 0 || ((uintptr_t)d_rgba_out & 15u) != 0 || ((uintptr_t)d_planes->id & 3u) != 0 ||
        (((uintptr_t)d_planes->position | (uintptr_t)d_planes->normal | (uintptr_t)d_variance | (uintptr_t)d_variance_out) & 7u) != 0)
        return fail(NDT_E_INVALID, "%s: misaligned: the images to 16 bytes, the planes to their elements", who);
    HIP_TRY(hipSetDevice(ctx->device));
    DenoiseState &dn = ctx->denoise;
    dn.launches = 0;
    dn.iterations = 0;
    dn.ms = 0.0;
    if ((rc = viterate(ctx, who, d_rgba_in, d_variance, *d_planes, dims, width, rows, d, d_rgba_out, d_variance_out))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return collect_ms(ctx);
}

extern "C" int ndt_hip_render_vdenoised_device(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, void *d_rgba,
                                               ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_vdenoised_device";
    ndt_vdenoise_params d;
    FrameView v;
    int rc = vrefuse(who, ctx, p, vp, d_rgba, &d, &v);
    if (rc) return rc;
    if (((uintptr_t)d_rgba & 15u) != 0) return fail(NDT_E_INVALID, "%s: misaligned: the image must be aligned to 16 bytes", who);
    return render_vdenoised(who, ctx, p, d, v.rows, d_rgba, stats);
}

extern "C" int ndt_hip_render_vdenoised(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, double *rgba,
                                        ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_vdenoised";
    ndt_vdenoise_params d;
    FrameView v;
    int rc = vrefuse(who, ctx, p, vp, rgba, &d, &v);
    if (rc) return rc;
    if ((rc = render_vdenoised_own(who, ctx, p, d, stats, &v))) return rc;
    return deliver_doubles(ctx, v, rgba, nullptr);
}

extern "C" int ndt_hip_render_vdenoised_rgba8(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, uint8_t *rgba8,
                                              ndt_render_stats *stats)
{
    const char *who = "ndt_hip_render_vdenoised_rgba8";
    ndt_vdenoise_params d;
    FrameView v;
    int rc = vrefuse(who, ctx, p, vp, rgba8, &d, &v);
    if (rc) return rc;
    if ((rc = render_vdenoised_own(who, ctx, p, d, stats, &v))) return rc;
    return deliver_rgba8(ctx, who, v, ctx->denoise.d_rgba8, rgba8);
}

extern "C" int ndt_hip_render_vdenoised_png(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, uint8_t *png, int64_t cap,
                                            ndt_png_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_vdenoised_png";
    ndt_vdenoise_params d;
    FrameView v;
    int rc = vrefuse(who, ctx, p, vp, png, &d, &v);
    if (rc) return rc;
    if ((rc = refuse_png(who, p->width, v.rows, 4))) return rc;
    if ((rc = render_vdenoised_own(who, ctx, p, d, render_stats, &v))) return rc;
    return deliver_png(ctx, who, v, ctx->denoise.d_rgba8, png, cap, stats);
}

extern "C" int ndt_hip_render_vdenoised_jpeg(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, const ndt_jpeg_params *jp,
                                             uint8_t *jpg, int64_t cap, ndt_jpeg_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_vdenoised_jpeg";
    ndt_vdenoise_params d;
    FrameView v;
    int rc = vrefuse(who, ctx, p, vp, jpg, &d, &v);
    if (rc) return rc;
    if ((rc = refuse_jpeg(who, p->width, v.rows, jp))) return rc;
    if ((rc = render_vdenoised_own(who, ctx, p, d, render_stats, &v))) return rc;
    return deliver_jpeg(ctx, who, v, ctx->denoise.d_rgba8, jp, jpg, cap, stats);
}

extern "C" int ndt_hip_render_vdenoised_exr(ndt_hip_ctx *ctx, const ndt_render_params *p, const ndt_vdenoise_params *vp, const ndt_exr_params *ep,
                                            uint8_t *out, int64_t cap, ndt_exr_stats *stats, ndt_render_stats *render_stats)
{
    const char *who = "ndt_hip_render_vdenoised_exr";
    if (stats) *stats = ndt_exr_stats{};
    ndt_vdenoise_params d;
    FrameView v;
    int rc = vrefuse(who, ctx, p, vp, out, &d, &v);
    if (rc) return rc;
    if (ndt_hip_exr_bound(p->width, v.rows, ep, 0) < 0)
        return fail(NDT_E_INVALID, "%s: no EXR of %d x %d with these parameters (a pixel type other than 0, 1, 2, or samples beyond 2^31 - 1 bytes)", who,
                    p->width, v.rows);
    if ((rc = render_vdenoised_own(who, ctx, p, d, render_stats, &v))) return rc;
    return deliver_exr(ctx, v, ep, out, cap, stats);
}
