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
//
// `priority` mode: how the waves that share a SIMD progress relative to each other.  Every
// wave records HW_REG_HW_ID / XCC_ID and the 100 MHz real-time counter at entry and exit;
// the host groups the records by SIMD and reports, as medians over SIMDs, when each of a
// SIMD's waves finished as a fraction of its last one (in dispatch order and sorted), the
// mean residency (sum of wave lifetimes / (waves x launch span)) and whether the resident
// waves of a SIMD have distinct WAVE_ID & 3.  An outer iteration is 19 steps (two are a
// transition of the kernel's element group pair); with R > 0 the wave sets its priority to
// (slot + outer / R) & 3 every R outer iterations, slot = WAVE_ID & 3.  R < 0 is the falling
// staircase instead: priority min(3, (outer iterations left - 1) / -R), which needs no slot --
// 3 for most of the launch, then 2, 1 and 0 over the last three windows of -R iterations, so a
// wave that is ahead yields to the ones behind it until they have caught up.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off scripts/fp64bench.hip -o scripts/fp64bench
//   scripts/fp64bench [out.json]
//   scripts/fp64bench priority [out.json]
//   scripts/fp64bench one <waves per SIMD> <U: 0, 1, 4> <R: 0, 2, 4, 8, -8>     (one form alone, for counters)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

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

// ---- priority mode -------------------------------------------------------------------

struct WaveRec {
    unsigned hw_id, xcc_id;
    unsigned long long t0, t1;
};

// s_setprio takes an immediate: a four-way scalar switch on a wave-uniform value
__device__ __forceinline__ void set_priority(unsigned p)
{
    switch (p & 3u) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

constexpr int OUTER_STEPS = 19;

template <int E, bool FMA, int U, int R>
__global__ void __launch_bounds__(256) leap_rec(double *out, WaveRec *rec, double seed, double dt, int outer)
{
    const unsigned hw_id = __builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4);     // HW_REG_HW_ID
    const unsigned xcc_id = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20);    // HW_REG_XCC_ID
    const unsigned slot = hw_id & 3u;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    double q[E], p[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        q[i] = seed * (double)(threadIdx.x * 31 + i * 7 + blockIdx.x + 1) * 1.2345678901234e-3;
        p[i] = seed * (double)(threadIdx.x * 17 + i * 3 + blockIdx.x + 2) * 0.9876543210987e-3;
    }
    const int inner = __builtin_amdgcn_readfirstlane(OUTER_STEPS + (outer < 0));         // a runtime trip count
#pragma unroll 1
    for (int o = 0; o < outer; ++o) {
        if (R > 0 && o % (R > 0 ? R : 1) == 0) set_priority(slot + (unsigned)(o / (R > 0 ? R : 1)));
        if (R < 0) {
            const int left = (outer - 1 - o) / (R < 0 ? -R : 1);
            set_priority(left < 3 ? left : 3);
        }
        if (U == 0) {
#pragma unroll
            for (int l = 0; l < OUTER_STEPS; ++l) step<E, FMA>(q, p, dt);
        } else if (U == 1) {
#pragma unroll 1
            for (int l = 0; l < inner; ++l) step<E, FMA>(q, p, dt);
        } else {
#pragma unroll U
            for (int l = 0; l < inner; ++l) step<E, FMA>(q, p, dt);
        }
    }
    if (R != 0) __builtin_amdgcn_s_setprio(0);
    // the arithmetic is complete before the exit stamp is taken
#pragma unroll
    for (int i = 0; i < E; ++i) asm volatile("" : "+v"(q[i]), "+v"(p[i]));
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < E; ++i) s += q[i] + p[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) {
        WaveRec r;
        r.hw_id = hw_id;
        r.xcc_id = xcc_id;
        r.t0 = t0;
        r.t1 = t1;
        rec[blockIdx.x * 4 + (threadIdx.x >> 6)] = r;
    }
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

static double median(std::vector<double> v)
{
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return (n & 1) ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]);
}

static void print_list(FILE *f, const std::vector<double> &v)
{
    fprintf(f, "[");
    for (size_t i = 0; i < v.size(); ++i) fprintf(f, "%s%.4f", i ? ", " : "", v[i]);
    fprintf(f, "]");
}

template <int E, bool FMA, int U, int R>
static void run_rec(int waves_per_simd, int outer, bool timed = true)
{
    const int blocks = 256 * waves_per_simd, nw = blocks * 4;
    double *out;
    WaveRec *rec;
    hipMalloc(&out, sizeof(double) * blocks * 256);
    hipMalloc(&rec, sizeof(WaveRec) * nw);
    hipMemset(rec, 0, sizeof(WaveRec) * nw);
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    const int reps = timed ? 10 : 1;
    for (int w = 0; w < (timed ? 3 : 0); ++w) leap_rec<E, FMA, U, R><<<blocks, 256>>>(out, rec, 1.0, 0.05, outer);
    hipEventRecord(a);
    for (int r = 0; r < reps; ++r) leap_rec<E, FMA, U, R><<<blocks, 256>>>(out, rec, 1.0, 0.05, outer);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    std::vector<WaveRec> h(nw);
    hipMemcpy(h.data(), rec, sizeof(WaveRec) * nw, hipMemcpyDeviceToHost);    // the last launch's records
    if (hipGetLastError() != hipSuccess) { fprintf(stderr, "HIP error\n"); exit(1); }
    const double t = ms * 1e-3 / reps;
    const double winst = (double)outer * OUTER_STEPS * E * (FMA ? 2 : 4) * waves_per_simd;
    const double tops = winst * 64 * 1024 / t * 1e-12;

    // XCC, SE, SH, CU (HW_ID bits 15:8) and SIMD (5:4) name the SIMD; WAVE_ID (3:0) the slot
    std::map<unsigned, std::vector<const WaveRec *>> simds;
    unsigned long long lo = ~0ull, hi = 0;
    double life = 0.0;
    for (const WaveRec &r : h) {
        simds[(r.xcc_id & 15u) << 16 | (r.hw_id & 0xff30u)].push_back(&r);
        lo = std::min(lo, r.t0);
        hi = std::max(hi, r.t1);
        life += (double)(r.t1 - r.t0);
    }
    const double residency = life / ((double)nw * (double)(hi - lo));
    std::vector<std::vector<double>> by_dispatch(waves_per_simd), sorted(waves_per_simd);
    int full = 0, distinct = 0;
    for (auto &kv : simds) {
        std::vector<const WaveRec *> &v = kv.second;
        if ((int)v.size() != waves_per_simd) continue;
        ++full;
        std::sort(v.begin(), v.end(), [](const WaveRec *x, const WaveRec *y) { return x->t0 < y->t0; });
        unsigned seen = 0;
        unsigned long long first = v[0]->t0, last = 0;
        for (const WaveRec *r : v) { seen |= 1u << (r->hw_id & 3u); last = std::max(last, r->t1); }
        if (__builtin_popcount(seen) == std::min(waves_per_simd, 4)) ++distinct;
        std::vector<double> f;
        for (const WaveRec *r : v) f.push_back((double)(r->t1 - first) / (double)(last - first));
        for (int k = 0; k < waves_per_simd; ++k) by_dispatch[k].push_back(f[k]);
        std::sort(f.begin(), f.end());
        for (int k = 0; k < waves_per_simd; ++k) sorted[k].push_back(f[k]);
    }
    std::vector<double> md, msr;
    for (int k = 0; k < waves_per_simd; ++k) { md.push_back(median(by_dispatch[k])); msr.push_back(median(sorted[k])); }
    char form[16];
    if (U == 0) snprintf(form, sizeof form, "19-step"); else snprintf(form, sizeof form, "U=%d", U);
    printf("E=%d %s %s waves/SIMD=%d R=%d: %.1f us, %.2f T lane-ops/s, residency %.3f, SIMDs %zu (%d with %d waves, "
           "%d of them with distinct WAVE_ID & 3), finish by dispatch order ", E, FMA ? "fma" : "exact", form,
           waves_per_simd, R, t * 1e6, tops, residency, simds.size(), full, waves_per_simd, distinct);
    print_list(stdout, md);
    printf(", sorted ");
    print_list(stdout, msr);
    printf("\n");
    fflush(stdout);
    if (js) {
        fprintf(js, "%s\n  {\"E\": %d, \"mode\": \"%s\", \"form\": \"%s\", \"waves_per_simd\": %d, \"rule\": \"%s\", \"R_outer_iterations\": %d, "
                    "\"outer\": %d, \"us\": %.1f, \"T_lane_ops_per_s\": %.3f, \"residency\": %.4f, \"simds_seen\": %zu, "
                    "\"simds_full\": %d, \"simds_distinct_slot\": %d, \"finish_by_dispatch_order\": ",
                js_first ? "" : ",", E, FMA ? "fma" : "exact", form, waves_per_simd,
                R == 0 ? "none" : (R > 0 ? "rotate" : "staircase"), R < 0 ? -R : R, outer, t * 1e6, tops, residency,
                simds.size(), full, distinct);
        print_list(js, md);
        fprintf(js, ", \"finish_sorted\": ");
        print_list(js, msr);
        fprintf(js, "}");
        js_first = false;
    }
    hipEventDestroy(a); hipEventDestroy(b);
    hipFree(out); hipFree(rec);
}

template <int U>
static void priority_rows(int outer)
{
    run_rec<8, false, U, 0>(1, outer);
    run_rec<8, false, U, 0>(4, outer);
    run_rec<8, false, U, 2>(4, outer);
    run_rec<8, false, U, 4>(4, outer);
    run_rec<8, false, U, 8>(4, outer);
    run_rec<8, false, U, -2>(4, outer);
    run_rec<8, false, U, -8>(4, outer);
    run_rec<8, false, U, -32>(4, outer);
    run_rec<8, false, U, 0>(4, outer);                     // the unrotated form again: its spread
}

template <int U>
static void one_form(int w, int R, int outer)
{
    if (R == 0) run_rec<8, false, U, 0>(w, outer, false);
    else if (R == 2) run_rec<8, false, U, 2>(w, outer, false);
    else if (R == 4) run_rec<8, false, U, 4>(w, outer, false);
    else if (R == 8) run_rec<8, false, U, 8>(w, outer, false);
    else run_rec<8, false, U, -8>(w, outer, false);
}

int main(int argc, char **argv)
{
    // 256 outer iterations of 19 steps: 128 transitions' worth for a pair of element groups, about
    // 1 ms at 4 waves per SIMD
    const int outer = 256;
    if (argc > 1 && !strcmp(argv[1], "one")) {
        if (argc != 5) { fprintf(stderr, "usage: fp64bench one <waves per SIMD> <U> <R>\n"); return 2; }
        const int w = atoi(argv[2]), U = atoi(argv[3]), R = atoi(argv[4]);
        if (w < 1 || w > 8 || (U != 0 && U != 1 && U != 4) || (R != 0 && R != 2 && R != 4 && R != 8 && R != -8)) {
            fprintf(stderr, "fp64bench one: waves 1..8, U in {0, 1, 4}, R in {0, 2, 4, 8, -8}\n");
            return 2;
        }
        for (int r = 0; r < 20; ++r) {
            if (U == 0) one_form<0>(w, R, outer); else if (U == 1) one_form<1>(w, R, outer); else one_form<4>(w, R, outer);
        }
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "priority")) {
        if (argc > 2) {
            js = fopen(argv[2], "w");
            if (!js) { perror(argv[2]); return 1; }
            fprintf(js, "{\"program\": \"scripts/fp64bench.hip priority\", \"outer\": %d, \"steps_per_outer\": %d, "
                        "\"launches_timed\": 10, \"rows\": [", outer, OUTER_STEPS);
        }
        priority_rows<1>(outer);
        priority_rows<4>(outer);
        priority_rows<0>(outer);
        if (js) { fprintf(js, "\n]}\n"); fclose(js); }
        return 0;
    }
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
