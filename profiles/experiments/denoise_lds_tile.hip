// denoise_lds_tile.hip -- experiment behind profiles/denoise_on_device.txt: does staging a tile and its halo in LDS pay for the
// a-trous iterations of step 1 and 2 (halo 2 and 4), against leaving the reuse of the 25 taps to the caches?
//
// A stand-alone program, not part of the library:
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o denoise_lds_tile profiles/experiments/denoise_lds_tile.hip
//     ./denoise_lds_tile
// k_plain is the text of k_denoise_atrous (ndt_amd/csrc/ndt_denoise.hip).  k_tile does the same arithmetic in the same order on a
// 32 x 8 pixel tile whose pixels and halo (2 * step on every side) it first copies to LDS, plane by plane: id, the four colour
// channels, N position and N normal planes, each [tile pixel] so that consecutive lanes read consecutive doubles.  Pixels that
// show nothing (id 0) are never a tap and are not staged.  The two kernels' images are compared bit for bit before any time is
// printed; a difference ends the run.  Synthetic 1920 x 1080 frames: ids in 64 x 64 blocks, a share of them 0; normals near one
// axis and hit points near the hyperplane across it, so that most taps of an object are taken.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>

#define TRY(expr)                                                                                 \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));                            \
            exit(1);                                                                              \
        }                                                                                         \
    } while (0)

constexpr int LANES = 256, TX = 32, TY = 8;

template <int N>
__global__ void __launch_bounds__(LANES) k_plain(const double2 *__restrict__ cur, double2 *__restrict__ next, const int *__restrict__ id,
                                                 const double *__restrict__ position, const double *__restrict__ normal, int width, int rows,
                                                 int step, double inv_c, double inv_p, int normal_power_log2)
{
    const long long n_pixels = (long long)rows * width;
    const long long p = (long long)blockIdx.x * LANES + threadIdx.x;
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

// LDS of a tile: (2 N + 4) planes of T doubles, then T ints
template <int N, int STEP> constexpr int tile_w() { return TX + 4 * STEP; }
template <int N, int STEP> constexpr int tile_h() { return TY + 4 * STEP; }
template <int N, int STEP> constexpr int tile_pixels() { return tile_w<N, STEP>() * tile_h<N, STEP>(); }
template <int N, int STEP> constexpr size_t tile_bytes() { return (size_t)tile_pixels<N, STEP>() * ((2 * N + 4) * sizeof(double) + sizeof(int)); }

template <int N, int STEP>
__global__ void __launch_bounds__(LANES) k_tile(const double2 *__restrict__ cur, double2 *__restrict__ next, const int *__restrict__ id,
                                                const double *__restrict__ position, const double *__restrict__ normal, int width, int rows,
                                                double inv_c, double inv_p, int normal_power_log2)
{
    constexpr int R = 2 * STEP, W = tile_w<N, STEP>(), T = tile_pixels<N, STEP>();
    extern __shared__ double lds[];
    double *s_pos = lds, *s_nrm = lds + N * T, *s_col = lds + 2 * N * T;
    int *s_id = (int *)(lds + (2 * N + 4) * T);
    const long long n_pixels = (long long)rows * width;
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * TX - R, y0 = (int)blockIdx.y * TY - R;
    for (int t = tid; t < T; t += LANES) {
        const int ty = t / W, tx = t - ty * W;
        const int gy = y0 + ty, gx = x0 + tx;
        int ident = 0;
        if (gy >= 0 && gy < rows && gx >= 0 && gx < width) {
            const long long g = (long long)gy * width + gx;
            ident = id[g];
            if (ident != 0) {
                const double2 rg = cur[2 * g], ba = cur[2 * g + 1];
                s_col[t] = rg.x;
                s_col[T + t] = rg.y;
                s_col[2 * T + t] = ba.x;
                s_col[3 * T + t] = ba.y;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    s_pos[k * T + t] = position[(long long)k * n_pixels + g];
                    s_nrm[k * T + t] = normal[(long long)k * n_pixels + g];
                }
            }
        }
        s_id[t] = ident;
    }
    __syncthreads();
    const int lx = tid & (TX - 1), ly = tid / TX;
    const int x = (int)blockIdx.x * TX + lx, y = (int)blockIdx.y * TY + ly;
    if (x >= width || y >= rows) return;
    const long long p = (long long)y * width + x;
    const int c = (ly + R) * W + lx + R;
    const int me = s_id[c];
    if (me == 0) {
        next[2 * p] = cur[2 * p];
        next[2 * p + 1] = cur[2 * p + 1];
        return;
    }
    const double p_r = s_col[c], p_g = s_col[T + c], p_b = s_col[2 * T + c], p_a = s_col[3 * T + c];
    double pn[N], pp[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        pn[k] = s_nrm[k * T + c];
        pp[k] = s_pos[k * T + c];
    }
    double num0 = 0.0, num1 = 0.0, num2 = 0.0, num3 = 0.0, den = 0.0;
#pragma unroll 1
    for (int j = 0; j < 5; ++j) {
        const double hj = j == 2 ? 0.375 : (j == 1 || j == 3) ? 0.25 : 0.0625;
        const int qy = y + (j - 2) * STEP;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double h = hj * (i == 2 ? 0.375 : (i == 1 || i == 3) ? 0.25 : 0.0625);
            const int qx = x + (i - 2) * STEP;
            double w = h;
            double q_r = p_r, q_g = p_g, q_b = p_b, q_a = p_a;
            if (j != 2 || i != 2) {
                if (qy < 0 || qy >= rows || qx < 0 || qx >= width) continue;
                const int q = c + (j - 2) * STEP * W + (i - 2) * STEP;      // inside the tile: the halo is 2 STEP wide
                if (s_id[q] != me) continue;
                double dd = 0.0, nd = 0.0, dot = 0.0;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double d = s_pos[k * T + q] - pp[k];
                    dd = dd + d * d;
                    nd = nd + pn[k] * d;
                    dot = dot + pn[k] * s_nrm[k * T + q];
                }
                double wn = dot > 0 ? dot : 0;
                for (int e = 0; e < normal_power_log2; ++e) wn = wn * wn;
                const double wp = dd > 0 ? 1.0 - ((nd * nd) / dd) * inv_p : 1.0;
                q_r = s_col[q];
                q_g = s_col[T + q];
                q_b = s_col[2 * T + q];
                q_a = s_col[3 * T + q];
                const double dr = q_r - p_r, dg = q_g - p_g, db = q_b - p_b;
                const double cc = (dr * dr + dg * dg) + db * db;
                const double wc = 1.0 / (1.0 + cc * inv_c);
                w = ((h * wn) * wp) * wc;
                if (!(w > 0)) continue;
            }
            num0 = num0 + w * q_r;
            num1 = num1 + w * q_g;
            num2 = num2 + w * q_b;
            num3 = num3 + w * q_a;
            den = den + w;
        }
    }
    next[2 * p] = make_double2(num0 / den, num1 / den);
    next[2 * p + 1] = make_double2(num2 / den, num3 / den);
}

struct Frame {
    int width, rows, dims;
    double *cur, *out_plain, *out_tile, *position, *normal;
    int *id;
};

template <typename F> static float median_ms(F launch, int reps)
{
    hipEvent_t a, b;
    TRY(hipEventCreate(&a));
    TRY(hipEventCreate(&b));
    std::vector<float> ms;
    for (int r = 0; r < reps + 2; ++r) {
        TRY(hipEventRecord(a, 0));
        launch();
        TRY(hipGetLastError());
        TRY(hipEventRecord(b, 0));
        TRY(hipEventSynchronize(b));
        float t = 0.0f;
        TRY(hipEventElapsedTime(&t, a, b));
        if (r >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    TRY(hipEventDestroy(a));
    TRY(hipEventDestroy(b));
    return ms[ms.size() / 2];
}

template <int N, int STEP> static void compare(const Frame &f, const char *what)
{
    const long long n_pixels = (long long)f.rows * f.width;
    const double sc = 0.25 / STEP, inv_c = 1.0 / (sc * sc), inv_p = 1.0 / (0.25 * 0.25);
    const size_t img = (size_t)n_pixels * 4 * sizeof(double), lds = tile_bytes<N, STEP>();
    TRY(hipFuncSetAttribute((const void *)k_tile<N, STEP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid_plain((unsigned)((n_pixels + LANES - 1) / LANES)), grid_tile((f.width + TX - 1) / TX, (f.rows + TY - 1) / TY);
    auto plain = [&] {
        hipLaunchKernelGGL(k_plain<N>, grid_plain, dim3(LANES), 0, 0, (const double2 *)f.cur, (double2 *)f.out_plain, (const int *)f.id,
                           (const double *)f.position, (const double *)f.normal, f.width, f.rows, STEP, inv_c, inv_p, 5);
    };
    auto tile = [&] {
        hipLaunchKernelGGL((k_tile<N, STEP>), grid_tile, dim3(LANES), lds, 0, (const double2 *)f.cur, (double2 *)f.out_tile, (const int *)f.id,
                           (const double *)f.position, (const double *)f.normal, f.width, f.rows, inv_c, inv_p, 5);
    };
    TRY(hipMemset(f.out_plain, 0xff, img));
    TRY(hipMemset(f.out_tile, 0xee, img));
    plain();
    tile();
    TRY(hipGetLastError());
    TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> a((size_t)n_pixels * 4), b((size_t)n_pixels * 4);
    TRY(hipMemcpy(a.data(), f.out_plain, img, hipMemcpyDeviceToHost));
    TRY(hipMemcpy(b.data(), f.out_tile, img, hipMemcpyDeviceToHost));
    long long differ = 0;
    for (size_t k = 0; k < a.size(); ++k) differ += a[k] != b[k];
    if (differ) {
        printf("%s N = %d step %d: %lld of %zu doubles differ between the plain and the tiled kernel: no time is taken\n", what, N, STEP, differ, a.size());
        exit(2);
    }
    // alternating, so that neither has the other's warm caches more than the other way round
    const float t_plain = median_ms(plain, 9), t_tile = median_ms(tile, 9), t_plain2 = median_ms(plain, 9), t_tile2 = median_ms(tile, 9);
    printf("%s N = %2d step %d: plain %.3f / %.3f ms, tiled through LDS (%zu bytes a workgroup) %.3f / %.3f ms (medians of 9, twice, alternating); the images agree bit for bit\n",
           what, N, STEP, t_plain, t_plain2, lds, t_tile, t_tile2);
    fflush(stdout);
}

template <int N> static void run(int width, int rows, double share_of_misses, const char *what)
{
    const long long n_pixels = (long long)rows * width;
    std::mt19937_64 rng(1234 + N);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::normal_distribution<double> gauss(0.0, 1.0);
    std::vector<int> id((size_t)n_pixels);
    std::vector<int> block(((rows + 63) / 64) * ((width + 63) / 64));
    for (int &b : block) b = uni(rng) < share_of_misses ? 0 : 1 + (int)(uni(rng) * 3.0);
    long long hit = 0;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < width; ++x) hit += (id[(size_t)y * width + x] = block[(y / 64) * ((width + 63) / 64) + x / 64]) != 0;
    std::vector<double> cur((size_t)n_pixels * 4), position((size_t)n_pixels * N), normal((size_t)n_pixels * N);
    for (double &v : cur) v = 2.0 * uni(rng);
    for (long long p = 0; p < n_pixels; ++p) {
        double len = 0.0, v[N];
        for (int k = 0; k < N; ++k) {
            v[k] = 0.15 * gauss(rng) + (k == 0 ? 1.0 : 0.0);
            len += v[k] * v[k];
            position[(size_t)k * n_pixels + p] = gauss(rng) * (k == 0 ? 0.05 : 1.0);
        }
        for (int k = 0; k < N; ++k) normal[(size_t)k * n_pixels + p] = v[k] / sqrt(len);
    }
    Frame f{ width, rows, N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    const size_t img = (size_t)n_pixels * 4 * sizeof(double), vec = (size_t)n_pixels * N * sizeof(double);
    TRY(hipMalloc(&f.cur, img));
    TRY(hipMalloc(&f.out_plain, img));
    TRY(hipMalloc(&f.out_tile, img));
    TRY(hipMalloc(&f.position, vec));
    TRY(hipMalloc(&f.normal, vec));
    TRY(hipMalloc(&f.id, (size_t)n_pixels * sizeof(int)));
    TRY(hipMemcpy(f.cur, cur.data(), img, hipMemcpyHostToDevice));
    TRY(hipMemcpy(f.position, position.data(), vec, hipMemcpyHostToDevice));
    TRY(hipMemcpy(f.normal, normal.data(), vec, hipMemcpyHostToDevice));
    TRY(hipMemcpy(f.id, id.data(), (size_t)n_pixels * sizeof(int), hipMemcpyHostToDevice));
    printf("%s: %d x %d, N = %d, %.1f %% of the pixels hit\n", what, width, rows, N, 100.0 * hit / n_pixels);
    compare<N, 1>(f, what);
    compare<N, 2>(f, what);
    TRY(hipFree(f.cur));
    TRY(hipFree(f.out_plain));
    TRY(hipFree(f.out_tile));
    TRY(hipFree(f.position));
    TRY(hipFree(f.normal));
    TRY(hipFree(f.id));
}

int main()
{
    // a small odd frame first: partial tiles on both edges, the comparison alone matters
    run<4>(333, 77, 0.2, "odd");
    run<12>(131, 45, 0.2, "odd");
    run<4>(1920, 1080, 0.2, "mostly hit");
    run<8>(1920, 1080, 0.2, "mostly hit");
    run<12>(1920, 1080, 0.2, "mostly hit");
    run<4>(1920, 1080, 0.9, "mostly missed");
    run<8>(1920, 1080, 0.9, "mostly missed");
    return 0;
}
