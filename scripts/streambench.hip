// The HBM streams of the C2 launch of hmc_gauss_persist_kernel<16, ..., WIDE> and nothing else:
// what rate this read + write traffic shape moves, and which knob changes it.  4096 waves in
// workgroups of 4, all resident (4 per SIMD); a wave owns one 8 KiB row per "transition" in
// each of two 2 GiB buffers, the transition stride is C D 8 = 32 MiB, 64 transitions per launch
// walk each buffer once, so the next launch finds nothing of it in the 256 MiB Infinity Cache.
// Per transition a wave issues two groups of 4 x 16 bytes per lane of loads (1 KiB per wave
// instruction), the second half a transition after the first and each a half transition before
// its values are used -- the kernel's 2-deep momentum ring -- and 8 x 16 bytes per lane of
// stores at the end.  The loaded values are added into the 16 doubles per lane that the stores
// write (what keeps both alive); a delay loop of `delay` x 8 VALU instructions after each
// group stands in for the trajectory: 0 = flat out, 47 = the 751 instructions per wave and
// transition of FMA mode, 87 = the 1391 of EXACT mode; kind 0 = v_add_u32 (the chip at its
// memory-side limit alone), kind 1 = v_fma_f64 on eight independent chains, a group's eight
// elements (the FP64 pipe's power as well).
//
// One knob at a time (scripts/streambench.py holds the table and what was expected of each):
//   ld, st   cache policy of the loads / the stores: 0 plain, 1 __builtin_nontemporal_* (`nt`
//            on gfx950: check with -S); through a buffer resource, where the builtin takes the
//            bits: 2 plain (the control of 3..5), 3 sc1, 4 sc0 sc1, 5 nt
//   stil     the 8 stores of transition s not back to back at its end but two behind each of
//            the first 4 loads of transition s + 1 (unconditionally, so that no branch splits
//            them: transition 0 stores its zeros, the last transition's values stay unstored,
//            the bytes per launch are the baseline's)
//   burst    the 8 loads of a transition as one 8 KiB group a whole transition ahead
//   slab     workgroup b -> chains by contiguous slabs per XCD (b % 8 is the XCD under round-robin
//            dispatch) instead of 32 KiB pieces round-robin over the eight XCDs
//   skew     the waves of a SIMD (HW_ID wave id & 3) work `skew` / 3 transitions apart: slot k
//            starts at transition k skew / 3 and wraps, so every wave still moves every byte
//            of its rows once and the launch is no longer, but the 32 MiB regions open at a
//            time are those of a SIMD whose oldest wave runs that far ahead
//   prio     the kernel's falling staircase of wave priority, min(3, (transitions left - 1) / 4):
//            it levels the waves of a SIMD over the last 16 transitions (gauss_wave_priority)
// Every wave records the 100 MHz counter at entry and exit: `finish` is when the waves ended
// as a fraction of the launch (5 % / 50 % quantile), i.e. how level they ran on their own.
//
//   hipcc --offload-arch=gfx950 -O3 scripts/streambench.hip -o scripts/streambench
//   scripts/streambench run <rounds> <launches per window> <spec> [<spec> ...]   (candidates take turns)
//   scripts/streambench one <launches> <spec>                                    (one form alone, for counters)
//   spec = name,ld,st,stil,burst,slab,skew,delay,kind,prio
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int C = 4096, D = 1024, NT = 64;           // chains (= waves), doubles per row, transitions per launch
constexpr long long CD = (long long)C * D;           // the transition stride in doubles
constexpr size_t BYTES = (size_t)NT * CD * 8;         // 2 GiB per buffer
constexpr double COPY_TBS = 6.29;                    // what a plain copy with the same 50/50 mix moves
static_assert(BYTES == (size_t)1 << 31, "the buffer resource's num_records below");

typedef double d2 __attribute__((ext_vector_type(2)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
enum { PLAIN = 0, NTB = 1, BUF = 2, BUF_SC1 = 3, BUF_SC0SC1 = 4, BUF_NT = 5 };
constexpr int buf_aux(int pol) { return pol == BUF_SC1 ? 16 : pol == BUF_SC0SC1 ? 17 : pol == BUF_NT ? 2 : 0; }

struct Args {
    const double *src;
    double *dst;
    unsigned long long *t0, *t1;
    int slab, skew, delay, kind, prio;
};

// element index `e` (in doubles, 16-byte aligned) of the buffer
template <int POL>
__device__ __forceinline__ d2 ld16(const double *p, __amdgpu_buffer_rsrc_t r, long long e)
{
    if constexpr (POL == PLAIN) return *reinterpret_cast<const d2 *>(p + e);
    else if constexpr (POL == NTB) return __builtin_nontemporal_load(reinterpret_cast<const d2 *>(p + e));
    else return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(r, (unsigned)(e * 8), 0, buf_aux(POL)));
}
template <int POL>
__device__ __forceinline__ void st16(double *p, __amdgpu_buffer_rsrc_t r, long long e, d2 v)
{
    if constexpr (POL == PLAIN) *reinterpret_cast<d2 *>(p + e) = v;
    else if constexpr (POL == NTB) __builtin_nontemporal_store(v, reinterpret_cast<d2 *>(p + e));
    else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), r, (unsigned)(e * 8), 0, buf_aux(POL));
}

__device__ __forceinline__ void delay(int n, int kind, unsigned &y, double (&x)[8])
{
    if (kind == 0) {
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int k = 0; k < 8; ++k) asm volatile("v_add_u32 %0, 1, %0" : "+v"(y));
        }
    } else {
        const double c = -1.0, d = 0.3;                          // x <-> 0.3 - x: bounded, the operands keep toggling
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int k = 0; k < 8; ++k) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(x[k]) : "v"(c), "v"(d));
        }
    }
}

// s_setprio takes an immediate: a four-way scalar switch on a wave-uniform value
__device__ __forceinline__ void set_priority(int p)
{
    switch (p & 3) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

template <int LD, int ST, bool STIL, bool BURST>
__global__ void __launch_bounds__(256) stream_kernel(const Args a)
{
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    int b = blockIdx.x;
    if (a.slab) {
        // XCD x = b % 8 takes blocks [start_x, start_x + n_x): every block exactly once, whatever the grid
        const int G = gridDim.x, x = b & 7, qq = G >> 3, rr = G & 7;
        b = x * qq + (x < rr ? x : rr) + (b >> 3);
    }
    const int wave = b * 4 + wib;
    if (wave >= C) return;
    const unsigned hw_id = __builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4);     // HW_REG_HW_ID
    const int off = (int)(hw_id & 3u) * a.skew / 3;
    if (lane == 0) a.t0[wave] = __builtin_amdgcn_s_memrealtime();
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.src, 0, (int)0x80000000u, 0x00027000);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void *)a.dst, 0, (int)0x80000000u, 0x00027000);
    const long long row = (long long)wave * D + 2 * lane;          // + 128 r, r = 0..7: < C D
    auto tt = [&](int s) { return (long long)((s + off) & (NT - 1)) * CD + row; };

    d2 q[8], pa[4], pb[4], nx[BURST ? 8 : 1];
    unsigned y = lane;
    double x[8] = {0.25 + lane, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0};
#pragma unroll
    for (int r = 0; r < 8; ++r) q[r] = d2{0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) pa[r] = ld16<LD>(a.src, rs, tt(0) + 128 * r);
    if (BURST) {
#pragma unroll
        for (int r = 0; r < 4; ++r) pb[r] = ld16<LD>(a.src, rs, tt(0) + 128 * (4 + r));
    }
#pragma unroll 1
    for (int s = 0; s < NT; ++s) {
        if (a.prio) {
            const int left = (NT - 1 - s) / 4;
            set_priority(left < 3 ? left : 3);
        }
        const long long pc = tt(s), pn = tt(s + 1 < NT ? s + 1 : s), pv = tt(s > 0 ? s - 1 : 0);
        if (BURST) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                nx[r] = ld16<LD>(a.src, rs, pn + 128 * r);
                if (STIL) st16<ST>(a.dst, rd, pv + 128 * r, q[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pb[r] = ld16<LD>(a.src, rs, pc + 128 * (4 + r));
                if (STIL) {
                    st16<ST>(a.dst, rd, pv + 128 * (2 * r), q[2 * r]);
                    st16<ST>(a.dst, rd, pv + 128 * (2 * r + 1), q[2 * r + 1]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            q[r] += pa[r];
            asm volatile("" ::"v"(q[r]));                         // used here, not sunk below the delay
        }
        delay(a.delay, a.kind, y, x);
        __builtin_amdgcn_sched_barrier(0);
        if (!BURST) {
#pragma unroll
            for (int r = 0; r < 4; ++r) pa[r] = ld16<LD>(a.src, rs, pn + 128 * r);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            q[4 + r] += pb[r];
            asm volatile("" ::"v"(q[4 + r]));
        }
        delay(a.delay, a.kind, y, x);
        __builtin_amdgcn_sched_barrier(0);
        if (BURST) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pa[r] = nx[r];
                pb[r] = nx[4 + r];
            }
        }
        if (!STIL) {
#pragma unroll
            for (int r = 0; r < 8; ++r) st16<ST>(a.dst, rd, pc + 128 * r, q[r]);
        }
    }
    if (a.prio) __builtin_amdgcn_s_setprio(0);
    if (lane == 0) a.t1[wave] = __builtin_amdgcn_s_memrealtime() + (y == 0xffffffffu) + (x[0] + x[1] + x[2] + x[3] + x[4] + x[5] + x[6] + x[7] == -1.0);
}

__global__ void fill_kernel(double *p, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long h = i * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 32;
        p[i] = ((double)(h >> 11) * 0x1p-53 - 0.5) * 3.4;        // zero buffers flatter the clock
    }
}

struct Spec {
    std::string name;
    int ld, st, stil, burst, slab, skew, delay, kind, prio;
};

static Spec parse(const char *s)
{
    Spec c;
    char name[128];
    if (sscanf(s, "%127[^,],%d,%d,%d,%d,%d,%d,%d,%d,%d", name, &c.ld, &c.st, &c.stil, &c.burst, &c.slab, &c.skew,
               &c.delay, &c.kind, &c.prio) != 10 || c.skew < 0 || c.skew > 63 || c.delay < 0) {
        fprintf(stderr, "bad spec %s\n", s);
        exit(2);
    }
    c.name = name;
    return c;
}

typedef void (*Kern)(const Args);
static Kern pick(const Spec &c)
{
#define POL(L, S) if (c.ld == L && c.st == S && !c.stil && !c.burst) return stream_kernel<L, S, false, false>;
#define SHAPE(L, S) POL(L, S) \
    if (c.ld == L && c.st == S && c.stil && !c.burst) return stream_kernel<L, S, true, false>; \
    if (c.ld == L && c.st == S && !c.stil && c.burst) return stream_kernel<L, S, false, true>; \
    if (c.ld == L && c.st == S && c.stil && c.burst) return stream_kernel<L, S, true, true>;
    SHAPE(PLAIN, PLAIN) SHAPE(NTB, PLAIN) SHAPE(PLAIN, NTB) SHAPE(NTB, NTB)
    POL(BUF, BUF) POL(BUF_SC1, BUF) POL(BUF, BUF_SC1) POL(BUF_SC1, BUF_SC1) POL(BUF_SC0SC1, BUF_SC0SC1)
    POL(BUF_NT, BUF_NT) POL(BUF, BUF_SC0SC1) POL(BUF_SC0SC1, BUF)
#undef SHAPE
#undef POL
    fprintf(stderr, "%s: this combination is not built\n", c.name.c_str());
    exit(2);
}

static void launch(const Spec &c, Args a)
{
    a.slab = c.slab; a.skew = c.skew; a.delay = c.delay; a.kind = c.kind; a.prio = c.prio;
    pick(c)<<<C / 4, 256>>>(a);
}

static double quantile(std::vector<double> v, double f)
{
    std::sort(v.begin(), v.end());
    return v[(size_t)(f * (v.size() - 1) + 0.5)];
}

int main(int argc, char **argv)
{
    if (argc < 4 || (strcmp(argv[1], "run") && strcmp(argv[1], "one"))) {
        fprintf(stderr, "usage: streambench run <rounds> <window> <spec>... | one <launches> <spec>\n");
        return 2;
    }
    const bool one = !strcmp(argv[1], "one");
    const int rounds = one ? 1 : atoi(argv[2]), window = atoi(argv[one ? 2 : 3]);
    std::vector<Spec> specs;
    for (int i = one ? 3 : 4; i < argc; ++i) specs.push_back(parse(argv[i]));
    if (specs.empty() || rounds < 1 || window < 1) return 2;
    for (auto &c : specs) pick(c);

    Args a;
    double *src, *dst;
    CK(hipMalloc(&src, BYTES));
    CK(hipMalloc(&dst, BYTES));
    CK(hipMalloc(&a.t0, C * 8));
    CK(hipMalloc(&a.t1, C * 8));
    a.src = src; a.dst = dst;
    fill_kernel<<<4096, 256>>>(src, BYTES / 8);
    fill_kernel<<<4096, 256>>>(dst, BYTES / 8);
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));

    if (one) {
        for (int i = 0; i < window; ++i) launch(specs[0], a);
        CK(hipDeviceSynchronize());
        CK(hipGetLastError());
        return 0;
    }
    std::vector<std::vector<double>> us(specs.size());
    for (size_t k = 0; k < specs.size(); ++k) {                  // warm-up: one window each
        for (int i = 0; i < window; ++i) launch(specs[k], a);
    }
    CK(hipDeviceSynchronize());
    for (int r = 0; r < rounds; ++r) {
        for (size_t k = 0; k < specs.size(); ++k) {
            CK(hipEventRecord(e0));
            for (int i = 0; i < window; ++i) launch(specs[k], a);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            us[k].push_back(ms * 1e3 / window / NT);
        }
    }
    CK(hipGetLastError());
    const double mb = 16.0 * D * C;                              // bytes per transition
    std::vector<unsigned long long> t0(C), t1(C);
    for (size_t k = 0; k < specs.size(); ++k) {
        const Spec &c = specs[k];
        launch(c, a);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(t0.data(), a.t0, C * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(t1.data(), a.t1, C * 8, hipMemcpyDeviceToHost));
        const unsigned long long lo = *std::min_element(t0.begin(), t0.end()), hi = *std::max_element(t1.begin(), t1.end());
        std::vector<double> fin(C);
        for (int w = 0; w < C; ++w) fin[w] = (double)(t1[w] - lo) / (double)(hi - lo);
        const double med = quantile(us[k], 0.5), mn = quantile(us[k], 0.0), mx = quantile(us[k], 1.0);
        printf("{\"name\": \"%s\", \"ld\": %d, \"st\": %d, \"stil\": %d, \"burst\": %d, \"slab\": %d, \"skew\": %d, "
               "\"delay\": %d, \"kind\": %d, \"prio\": %d, \"us_per_transition\": [%.4f, %.4f, %.4f], \"TBps\": [%.4f, %.4f, %.4f], "
               "\"of_copy_ceiling\": %.4f, \"finish_q05_q50\": [%.3f, %.3f], \"windows\": %d, \"launches_per_window\": %d}\n",
               c.name.c_str(), c.ld, c.st, c.stil, c.burst, c.slab, c.skew, c.delay, c.kind, c.prio, med, mn, mx,
               mb / med * 1e-6, mb / mx * 1e-6, mb / mn * 1e-6, mb / med * 1e-6 / COPY_TBS,
               quantile(fin, 0.05), quantile(fin, 0.5), rounds, window);
    }
    return 0;
}
