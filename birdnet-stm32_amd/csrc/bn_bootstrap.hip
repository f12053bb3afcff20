// bn_bootstrap.hip — the bootstrap behind `evaluate`'s per-class average-precision intervals (bn_bootstrap_*).
//
// The reference draws, per class and resample, n row indices with numpy's `rng.integers(0, n, size=n)` and calls scikit-learn's
// average_precision_score on the picked rows (birdnet_stm32/evaluation/metrics.py:239-318): 100 000 sorts for 100 classes x 1000
// resamples.  Here a resample is a vector of multiplicities over the rows; each class is sorted once (bn_rank_orders) and the average
// precision of a resample is a weighted prefix sum over that fixed order.  The draws are numpy's own, reproduced on the device
// (birdnet_stm32/evaluation/bootstrap.py restates the stream and is the specification):
//   PCG64      state = state * MULT + inc (mod 2^128); output = (hi ^ lo) rotated right by state >> 122, of the NEW state
//   32-bit     raw position 2 q is the low half of the q-th output, 2 q + 1 its high half
//   Lemire     m = x * n; rejected when (m mod 2^32) < thr = (2^32 - n) mod n, else the value is m >> 32
// Rejection depends on the raw value alone, so a resample is a raw range [p0, p1) with its rejected entries skipped.  The rejection scan
// finds those entries; the host turns them into one range per resample (`resample_ranges`).
//
// Kernels:
//   bootstrap_table_kernel     (A^(2^i), inc * (A^(2^i) - 1) / (A - 1)) for i < 64: the jump-ahead by 2^i steps, 2 KiB
//   bootstrap_reject_kernel    raw positions whose value is rejected, appended with an integer atomic (order is the host's business)
//   bootstrap_prepare_kernel   per class: (row | truth << 30 | end of a run of equal scores << 31) along the descending order, stored so that
//                              thread t's elements t * per .. t * per + per - 1 are read as word [i * 256 + t] (coalesced)
//   bootstrap_resample_kernel  one workgroup per (class, resample): multiplicities in LDS, then the average precision
//
// Float64 throughout the average precision; every term is the expression scikit-learn evaluates, (tps / K - tps_prev / K) * (tps / seen)
// with each operation rounded on its own, so only the ORDER of the final sum differs from numpy's pairwise sum (at most 2 n 2^-53 off).
// The sum runs in a fixed order (thread, then a shuffle tree, then the four waves): no floating-point atomics, same bits on every run.
#include "bn_device.h"
#include "bn_kernels.h"

namespace bn {
namespace {

struct U128 {
    unsigned long long hi, lo;
};

constexpr unsigned long long kMultHi = 0x2360ED051FC65DA4ULL, kMultLo = 0x4385DF649FCCF645ULL;
constexpr int kRejectOutputs = 32;    // 64-bit outputs per thread of the rejection scan
constexpr int kScratchWords = 32;     // front of the resample kernel's LDS: the block scans' and the final sum's per-wave values

// a * m + c (mod 2^128)
__device__ __forceinline__ U128 mul_add(U128 a, U128 m, U128 c) {
    const unsigned long long lo = a.lo * m.lo;
    const unsigned long long hi = __umul64hi(a.lo, m.lo) + a.hi * m.lo + a.lo * m.hi;
    U128 r;
    r.lo = lo + c.lo;
    r.hi = hi + c.hi + (r.lo < lo ? 1ULL : 0ULL);
    return r;
}

__device__ __forceinline__ U128 pcg_step(U128 s, U128 inc) { return mul_add(s, U128{kMultHi, kMultLo}, inc); }

__device__ __forceinline__ unsigned long long xsl_rr(U128 s) {
    const unsigned long long x = s.hi ^ s.lo;
    const unsigned rot = (unsigned)(s.hi >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

// table[i] = (mult.hi, mult.lo, plus.hi, plus.lo) of 2^i steps
__global__ __launch_bounds__(64) void bootstrap_table_kernel(U128 inc, ulonglong4* __restrict__ table) {
    if (threadIdx.x != 0) return;
    U128 m{kMultHi, kMultLo}, p = inc;
    for (int i = 0; i < 64; ++i) {
        table[i] = make_ulonglong4(m.hi, m.lo, p.hi, p.lo);
        U128 m1 = m;   // m + 1
        m1.lo += 1;
        m1.hi += m1.lo == 0 ? 1ULL : 0ULL;
        p = mul_add(p, m1, U128{0, 0});
        m = mul_add(m, m, U128{0, 0});
    }
}

// the state `delta` steps on
__device__ __forceinline__ U128 pcg_jump(U128 s, unsigned long long delta, const ulonglong4* __restrict__ table) {
    for (int i = 0; delta; ++i, delta >>= 1)
        if (delta & 1) {
            const ulonglong4 t = table[i];
            s = mul_add(s, U128{t.x, t.y}, U128{t.z, t.w});
        }
    return s;
}

__global__ __launch_bounds__(256) void bootstrap_reject_kernel(U128 state, U128 inc, const ulonglong4* __restrict__ table, unsigned n, unsigned thr,
                                                               long long p_begin, long long p_end, unsigned* __restrict__ counter,
                                                               long long* __restrict__ list, unsigned cap) {
    const long long q_end = (p_end + 1) >> 1;
    long long q = (p_begin >> 1) + ((long long)blockIdx.x * 256 + threadIdx.x) * kRejectOutputs;
    if (q >= q_end) return;
    const long long qe = q + kRejectOutputs < q_end ? q + kRejectOutputs : q_end;
    U128 s = pcg_jump(state, (unsigned long long)q, table);
    for (; q < qe; ++q) {
        s = pcg_step(s, inc);
        const unsigned long long v = xsl_rr(s);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned x = h ? (unsigned)(v >> 32) : (unsigned)v;
            const long long p = 2 * q + h;
            if (p >= p_begin && p < p_end && (unsigned)((unsigned long long)x * n) < thr) {
                const unsigned at = atomicAdd(counter, 1u);   // counts past `cap` too: the host sees the overflow
                if (at < cap) list[at] = p;
            }
        }
    }
}

__global__ __launch_bounds__(256) void bootstrap_prepare_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ truth, int n, int C,
                                                                const int* __restrict__ cols, const int* __restrict__ classes, int per,
                                                                unsigned* __restrict__ prep) {
    const int ci = blockIdx.y;
    int c = classes[ci];   // (device tables the host cannot see: clamped, so a bad one gives a wrong result, never a stray read)
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);
    const int* order = cols + (long)c * n;
    unsigned* out = prep + (long)ci * per * 256;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        int row = order[k];
        row = row < 0 ? 0 : (row >= n ? n - 1 : row);
        const float s = scores[(long)row * C + c];
        bool last = k == n - 1;
        if (!last) {
            int next = order[k + 1];
            next = next < 0 ? 0 : (next >= n ? n - 1 : next);
            last = scores[(long)next * C + c] != s;
        }
        const unsigned word = (unsigned)row | (truth[(long)row * C + c] ? 1u << 30 : 0u) | (last ? 1u << 31 : 0u);
        out[(k % per) * 256 + k / per] = word;
    }
}

// exclusive prefix sum over the workgroup's 256 threads in thread order; scratch: 4 values, free again on return
__device__ __forceinline__ unsigned long long block_scan_add(unsigned long long v, unsigned long long* scratch, unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) scratch[wave] = inc;
    lds_barrier();
    unsigned long long base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned long long x = scratch[w];
        if (w < wave) base += x;
        tot += x;
    }
    lds_barrier();
    *total = tot;
    return base + inc - v;
}

// exclusive prefix maximum (0 in front of the first thread)
__device__ __forceinline__ unsigned block_scan_max(unsigned v, unsigned* scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= d) inc = inc > o ? inc : o;
    }
    if (lane == 63) scratch[wave] = inc;
    lds_barrier();
    unsigned base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned x = scratch[w];
        if (w < wave && x > base) base = x;
    }
    lds_barrier();
    const unsigned before = __shfl_up(inc, 1);
    return lane == 0 ? base : (before > base ? before : base);
}

// One term of the average precision, each operation rounded on its own (a fused multiply-add would round the product into the sum)
__device__ __forceinline__ double ap_add_term(double acc, unsigned tps, unsigned tps_prev, unsigned seen, double K) {
#pragma clang fp contract(off)
    const double r1 = (double)tps / K, r0 = (double)tps_prev / K;
    const double precision = (double)tps / (double)seen;
    const double term = (r1 - r0) * precision;
    return acc + term;
}

__device__ __forceinline__ double add_f64(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

struct ResampleArgs {
    U128 state, inc;
    const ulonglong4* table;
    const long long* ranges;   // [resamples, 2] raw positions
    const unsigned* prep;      // [classes][per * 256] (bootstrap_prepare_kernel); unused with counts_out
    double* ap;                // [resamples]
    unsigned* counts_out;      // [resamples, n]: write the multiplicities and stop
    int n, per, B;
    unsigned thr;
};

__global__ __launch_bounds__(256) void bootstrap_resample_kernel(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned smem[];
    unsigned* cnt = smem + kScratchWords;   // (n + 1) / 2 words: two 16-bit multiplicities each (a multiplicity is <= n <= 32768)
    const int tid = threadIdx.x, n = a.n;
    const long r = blockIdx.x;
    for (int i = tid; i < (n + 1) >> 1; i += 256) cnt[i] = 0;
    long long p0 = a.ranges[2 * r], p1 = a.ranges[2 * r + 1];
    // a range holds n accepted values and the few rejected ones between them; a table that says otherwise gives wrong numbers, never a
    // long loop (the LDS index below is < n whatever the range is)
    if (p0 < 0) p0 = 0;
    if (p1 < p0) p1 = p0;
    if (p1 - p0 > 2LL * n + 64) p1 = p0 + 2LL * n + 64;
    lds_barrier();
    {
        const long long q0 = p0 >> 1, q1 = (p1 + 1) >> 1;
        const long long each = (q1 - q0 + 255) / 256;
        long long q = q0 + tid * each;
        const long long qe = q + each < q1 ? q + each : q1;
        if (q < qe) {
            U128 s = pcg_jump(a.state, (unsigned long long)q, a.table);
            for (; q < qe; ++q) {
                s = pcg_step(s, a.inc);
                const unsigned long long v = xsl_rr(s);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const unsigned long long m = (unsigned long long)(h ? (unsigned)(v >> 32) : (unsigned)v) * (unsigned)n;
                    const long long p = 2 * q + h;
                    if (p >= p0 && p < p1 && (unsigned)m >= a.thr) {
                        const unsigned row = (unsigned)(m >> 32);   // < n
                        atomicAdd(&cnt[row >> 1], 1u << ((row & 1u) * 16u));
                    }
                }
            }
        }
    }
    lds_barrier();
    if (a.counts_out) {
        unsigned* out = a.counts_out + r * n;
        for (int i = tid; i < n; i += 256) out[i] = (cnt[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
        return;
    }
    // ---- average precision along the class's descending order; thread t owns elements [t * per, t * per + per)
    const unsigned* pr = a.prep + (r / a.B) * ((long)a.per * 256);
    const int k0 = tid * a.per;
    const int mine = k0 >= n ? 0 : (n - k0 < a.per ? n - k0 : a.per);
    unsigned sw = 0, swt = 0, end_rel = 0;
    bool has_end = false;
    for (int i = 0; i < mine; ++i) {
        const unsigned word = pr[i * 256 + tid];
        const unsigned row = word & 0x3fffffffu;
        const unsigned w = (cnt[row >> 1] >> ((row & 1u) * 16u)) & 0xffffu;
        sw += w;
        swt += (word >> 30) & 1u ? w : 0u;
        if (word >> 31) {
            has_end = true;
            end_rel = swt;
        }
    }
    unsigned long long* scratch64 = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long total;
    const unsigned long long before = block_scan_add(((unsigned long long)sw << 32) | swt, scratch64, &total);
    const unsigned N = (unsigned)(total >> 32), K = (unsigned)total;
    unsigned seen = (unsigned)(before >> 32), tps = (unsigned)before;
    unsigned prev = block_scan_max(has_end ? tps + end_rel : 0u, smem);   // true positives at the last run end in front of this thread
    double acc = 0.0;
    const bool dropped = K == 0 || K == N;
    if (!dropped) {
        const double dK = (double)K;
        for (int i = 0; i < mine; ++i) {
            const unsigned word = pr[i * 256 + tid];
            const unsigned row = word & 0x3fffffffu;
            const unsigned w = (cnt[row >> 1] >> ((row & 1u) * 16u)) & 0xffffu;
            seen += w;
            tps += (word >> 30) & 1u ? w : 0u;
            if (word >> 31) {
                if (seen > 0) acc = ap_add_term(acc, tps, prev, seen, dK);
                prev = tps;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc = add_f64(acc, __shfl_down(acc, d));
    double* scratchf = reinterpret_cast<double*>(smem);
    if ((tid & 63) == 0) scratchf[tid >> 6] = acc;
    lds_barrier();
    if (tid == 0) {
        const double sum = add_f64(add_f64(add_f64(scratchf[0], scratchf[1]), scratchf[2]), scratchf[3]);
        a.ap[r] = dropped ? __longlong_as_double(0x7ff8000000000000LL) : sum;
    }
}

size_t resample_lds_bytes(int n) { return (size_t)kScratchWords * 4 + (size_t)((n + 1) / 2) * 4; }

}  // namespace

// Workspace: [table 2 KiB | counter 256 B | rejection list or prepared orders]
static constexpr size_t kBootHead = 2048 + 256;

size_t bootstrap_reject_workspace(long capacity) { return kBootHead + (size_t)capacity * 8; }

size_t bootstrap_ap_workspace(int n, int n_sel) {
    const size_t per = ((size_t)n + 255) / 256;
    return kBootHead + (size_t)n_sel * per * 256 * 4;
}

static void launch_table(const unsigned long long gen[4], void* d_work, hipStream_t s) {
    hipLaunchKernelGGL(bootstrap_table_kernel, dim3(1), dim3(64), 0, s, U128{gen[2], gen[3]}, (ulonglong4*)d_work);
}

// d_work: bootstrap_reject_workspace(capacity) bytes; afterwards the counter (unsigned, at byte 2048) holds the number of rejected positions in
// [p_begin, p_end) and the list (long long, at byte kBootHead) the first min(counter, capacity) found
void launch_bootstrap_reject(const unsigned long long gen[4], unsigned n, long long p_begin, long long p_end, void* d_work, long capacity, hipStream_t s) {
    char* w = (char*)d_work;
    launch_table(gen, d_work, s);
    (void)hipMemsetAsync(w + 2048, 0, 256, s);
    const unsigned thr = (unsigned)((0x100000000ULL - n) % n);
    const long long nq = ((p_end + 1) >> 1) - (p_begin >> 1);
    const long long per_block = 256LL * kRejectOutputs;
    const unsigned blocks = (unsigned)((nq + per_block - 1) / per_block);
    if (blocks == 0) return;
    hipLaunchKernelGGL(bootstrap_reject_kernel, dim3(blocks), dim3(256), 0, s, U128{gen[0], gen[1]}, U128{gen[2], gen[3]}, (const ulonglong4*)d_work, n, thr,
                       p_begin, p_end, (unsigned*)(w + 2048), (long long*)(w + kBootHead), (unsigned)capacity);
}

static bool launch_resample(const unsigned long long gen[4], int n, int B, long resamples, const long long* d_ranges, const unsigned* prep, double* d_ap,
                            unsigned* d_counts, void* d_work, hipStream_t s) {
    const size_t lds = resample_lds_bytes(n);
    if (lds > 64 * 1024 && !ensure_dynamic_lds(reinterpret_cast<const void*>(&bootstrap_resample_kernel), lds)) return false;
    ResampleArgs a;
    a.state = U128{gen[0], gen[1]};
    a.inc = U128{gen[2], gen[3]};
    a.table = (const ulonglong4*)d_work;
    a.ranges = d_ranges;
    a.prep = prep;
    a.ap = d_ap;
    a.counts_out = d_counts;
    a.n = n;
    a.per = (n + 255) / 256;
    a.B = B;
    a.thr = (unsigned)((0x100000000ULL - (unsigned)n) % (unsigned)n);
    hipLaunchKernelGGL(bootstrap_resample_kernel, dim3((unsigned)resamples), dim3(256), lds, s, a);
    return true;
}

// d_work: bootstrap_ap_workspace(n, 0) bytes
bool launch_bootstrap_counts(const unsigned long long gen[4], int n, int B, const long long* d_ranges, unsigned* d_counts, void* d_work, hipStream_t s) {
    launch_table(gen, d_work, s);
    return launch_resample(gen, n, B, B, d_ranges, nullptr, nullptr, d_counts, d_work, s);
}

// d_work: bootstrap_ap_workspace(n, n_sel) bytes
bool launch_bootstrap_ap(const unsigned long long gen[4], int n, int C, const float* d_scores, const unsigned char* d_truth, const int* d_cols,
                         const int* d_classes, int n_sel, int B, const long long* d_ranges, double* d_ap, void* d_work, hipStream_t s) {
    launch_table(gen, d_work, s);
    unsigned* prep = (unsigned*)((char*)d_work + kBootHead);
    const int per = (n + 255) / 256;
    const unsigned bx = (unsigned)((n + 255) / 256 < 64 ? (n + 255) / 256 : 64);
    hipLaunchKernelGGL(bootstrap_prepare_kernel, dim3(bx, (unsigned)n_sel), dim3(256), 0, s, d_scores, d_truth, n, C, d_cols, d_classes, per, prep);
    return launch_resample(gen, n, B, (long)n_sel * B, d_ranges, prep, d_ap, nullptr, d_work, s);
}

void preload_bootstrap() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&bootstrap_resample_kernel));
}

}  // namespace bn
