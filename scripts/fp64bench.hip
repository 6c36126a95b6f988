// FP64 VALU ceiling for the EXACT-mode leapfrog arithmetic on gfx950: the same
// mul/add sequence as hmc_gauss_persist_kernel's step loop, no memory traffic.
// Reports wave-instruction issue rate as an effective clock (instructions x 4
// cycles / SIMD / time) for 1..8 waves per SIMD and for random vs zero data
// (the latter shows how much of the limit is power, not issue slots).
//
// The step loop is unrolled by a compile-time factor U (U = 1: the bare loop,
// E x 4 instructions per taken back-edge) with the trip count a runtime value,
// so a remainder loop exists as it does in the kernel.  U = 0 is the kernel's
// L = 20 shape taken literally: 19 steps in straight line inside an outer loop
// (one taken back-edge per 19 x E x 4 instructions).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off scripts/fp64bench.hip -o scripts/fp64bench
//   scripts/fp64bench [out.json]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

template <int E, bool FMA>
__device__ __forceinline__ void step(double (&q)[E], double (&p)[E], double dt)
{
#pragma unroll
    for (int i = 0; i < E; ++i) {
        if (FMA) {
            q[i] = __builtin_fma(p[i], dt, q[i]);
            p[i] = __builtin_fma(-dt, q[i], p[i]);
        } else {
            q[i] = q[i] + p[i] * dt;
            p[i] = p[i] - dt * q[i];
        }
    }
}

template <int E, bool FMA, int U>
__global__ void __launch_bounds__(256) leap(double *out, double seed, double dt, int iters)
{
    double q[E], p[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        q[i] = seed * (double)(threadIdx.x * 31 + i * 7 + blockIdx.x + 1) * 1.2345678901234e-3;
        p[i] = seed * (double)(threadIdx.x * 17 + i * 3 + blockIdx.x + 2) * 0.9876543210987e-3;
    }
    if (U == 0) {
        for (int o = 0; o < iters / 19; ++o) {
#pragma unroll
            for (int l = 0; l < 19; ++l) step<E, FMA>(q, p, dt);
        }
    } else if (U == 1) {
#pragma unroll 1
        for (int l = 0; l < iters; ++l) step<E, FMA>(q, p, dt);
    } else {
#pragma unroll U
        for (int l = 0; l < iters; ++l) step<E, FMA>(q, p, dt);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < E; ++i) s += q[i] + p[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

static FILE *js = nullptr;
static bool js_first = true;

template <int E, bool FMA, int U>
static void run(int waves_per_simd, double seed, int iters, int rep_id = 0)
{
    const int blocks = 256 * waves_per_simd;             // 256 CUs x 4 SIMDs, 4 waves per block
    double *out;
    hipMalloc(&out, sizeof(double) * blocks * 256);
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    for (int w = 0; w < 3; ++w) leap<E, FMA, U><<<blocks, 256>>>(out, seed, 0.05, iters);
    hipEventRecord(a);
    const int reps = 20;
    for (int r = 0; r < reps; ++r) leap<E, FMA, U><<<blocks, 256>>>(out, seed, 0.05, iters);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    if (hipGetLastError() != hipSuccess) { fprintf(stderr, "HIP error\n"); exit(1); }
    const double t = ms * 1e-3 / reps;
    const int done = (U == 0) ? iters / 19 * 19 : iters;
    const double winst = (double)done * E * (FMA ? 2 : 4) * waves_per_simd;   // per SIMD
    const double tops = winst * 64 * 1024 / t * 1e-12, ghz = winst * 4 / t * 1e-9;
    char form[16];
    if (U == 0) snprintf(form, sizeof form, "19-step"); else snprintf(form, sizeof form, "U=%d", U);
    printf("E=%d %s %s waves/SIMD=%d data=%s: %.1f us, %.2f T lane-ops/s, effective issue clock %.2f GHz\n",
           E, FMA ? "fma" : "exact", form, waves_per_simd, seed == 0.0 ? "zero" : "random", t * 1e6,
           tops, ghz);
    fflush(stdout);
    if (js) {
        fprintf(js, "%s\n  {\"E\": %d, \"mode\": \"%s\", \"form\": \"%s\", \"waves_per_simd\": %d, \"data\": \"%s\", "
                    "\"repeat\": %d, \"us\": %.1f, \"T_lane_ops_per_s\": %.3f, \"issue_clock_GHz\": %.4f}",
                js_first ? "" : ",", E, FMA ? "fma" : "exact", form, waves_per_simd,
                seed == 0.0 ? "zero" : "random", rep_id, t * 1e6, tops, ghz);
        js_first = false;
    }
    hipEventDestroy(a); hipEventDestroy(b);
    hipFree(out);
}

template <int U>
static void sweep(int iters)
{
    for (double seed : {1.0, 0.0})
        for (int w : {1, 2, 4, 8}) run<8, false, U>(w, seed, iters);
}

int main(int argc, char **argv)
{
    const int iters = 19 * 1000;
    if (argc > 1) {
        js = fopen(argv[1], "w");
        if (!js) { perror(argv[1]); return 1; }
        fprintf(js, "{\"program\": \"scripts/fp64bench.hip\", \"iters\": %d, \"launches_timed\": 20, \"rows\": [", iters);
    }
    // the spread of the bare loop at the kernel's occupancy: three repeats, taken
    // before, between and after the sweeps so that a drift would show
    run<8, false, 1>(4, 1.0, iters, 1);
    sweep<1>(iters);
    sweep<2>(iters);
    run<8, false, 1>(4, 1.0, iters, 2);
    sweep<4>(iters);
    sweep<5>(iters);
    sweep<0>(iters);
    run<8, false, 1>(4, 1.0, iters, 3);
    run<16, false, 1>(4, 1.0, iters);
    run<8, true, 1>(4, 1.0, iters);
    run<8, true, 4>(4, 1.0, iters);
    run<8, true, 1>(4, 0.0, iters);
    if (js) { fprintf(js, "\n]}\n"); fclose(js); }
    return 0;
}
