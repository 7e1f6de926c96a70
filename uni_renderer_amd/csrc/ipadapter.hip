// IP-Adapter's decoupled cross-attention (Ye et al., arXiv 2308.06721; diffusers' IPAdapterAttnProcessor2_0) behind a
// cross-attention whose prompt half ur_attention has already written to o:
//   o[b][t][h*d : (h+1)*d] += scale * sum_j p_j * v_ip[b][j][h*d : (h+1)*d],   p = softmax_j(q[b][t][h] . k_ip[b][j][h])
// over the N <= 16 image tokens: a second softmax with its own normaliser, so it cannot ride in the 77-key launch.  One
// memory-bound pass: q is read once, o is read once and written once, all in 16-byte vectors; a sample's k_ip / v_ip
// (2 N C elements, at most 80 KB) are staged once per workgroup into LDS and read from there as 16-byte vectors.
//
// Thread mapping ("IP-Adapter"): one lane per 8-channel vector.  A head of the SD-1.x networks is VPD = d / 8 = 5,
// 10 or 20 vectors -- never a power of two -- but 60 is a multiple of all three, so a wave takes 60 / VPD whole (token, head)
// pairs on its lanes 0 .. 59 (lanes 60 .. 63 idle: 94 % of the lanes, every load and store a full 16-byte vector, and with a
// token-major q of ldq = C the 60 lanes read one contiguous 960-byte run).  The dot product of a head is reduced across its
// lanes in a fixed tree: 8 fmas per lane, log2(G) butterfly adds inside the aligned groups of G = VPD / 5 lanes, then the five
// group sums added left to right (five lane reads per score, whatever d is).  Every lane of a head ends with the same bits.
// No atomics.  The power-of-two widths (d = 32, 64, 128: VPD = G = 4, 8, 16, all 64 lanes) are the butterfly alone.
// flags bit 0 selects the alternative that was measured against it: one thread per (token, head) that walks the
// head's VPD vectors itself, with the SAME summation tree, so the two kernels produce the same bits.
//
// Work split: a group = the 4 x (64 / VPD) pairs the four waves of a workgroup take at once.  The launches are latency-bound (a
// few thousand short-lived workgroups), so every group gets its own workgroup until a launch has 4096 of them; longer walks keep
// the next group's q / o loads in flight (requested one group ahead, the first before the staging barrier).  Measured with the
// walk forced to 1 .. 16 groups through flags bits 8 .. 15: profiles/ip_adapter_ab.txt.
//
// Arithmetic, all fp32 in a fixed order: score_j as above (q already carries d^-1/2 log2 e: log2 units), m = max_j score_j,
// p_j = exp2(score_j - m), l = p_0 + p_1 + ..., acc = fma(p_j, v_j, acc) for j = 0 .. N - 1 from 0, w = scale * (1 / l) with a
// correctly rounded division, result = fma(acc, w, o), rounded once to the storage type.
#include <math.h>

#include "ur_launch.h"

namespace ur {

struct IpaArgs {
    void* o;
    const void* q;
    const void* k;
    const void* v;
    float scale;
    int T, N, H;
    int pairs;  // T * H (token, head) pairs of a sample
    int bps;    // workgroups per sample
    int iters;  // pair groups per workgroup
    int q_off;
    int64_t ldq, q_hstride, ldkv;
};

constexpr int IPA_NMAX = 16;
constexpr int IPA_THREAD_PER_HEAD = 1, IPA_WALK_SHIFT = 8;  // `flags` (include/ur_kernels.h)
constexpr int IPA_GROUPS_PER_WALK = 2048;  // groups in a launch per extra group a workgroup walks (the launcher, below)
constexpr int IPA_CMAX = 1280;  // H * d up to which a sample's keys and values fit the LDS at N = 16

// lanes of a wave that carry a vector (60 for VPD = 5, 10, 20), the butterfly width G = the largest power of two in VPD, and
// the VPD / G = 1 or 5 group sums that are added left to right
template <int VPD>
struct IpaGeom {
    static constexpr int LANES = (64 / VPD) * VPD, HPW = 64 / VPD, G = VPD & -VPD, R = VPD / G;
    static_assert(R == 1 || R == 5, "head widths: 8 * 2^k or 40 * 2^k");
};

template <typename T>
__device__ __forceinline__ void ipa_unpack(const typename Vec8<T>::type& r, float (&x)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (float)r[e];
}

template <typename T>
__device__ __forceinline__ float ipa_dot8(const float (&x)[8], const typename Vec8<T>::type& r) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(x[e], (float)r[e], s);
    return s;
}

// element offset of head h of token t inside a sample of q: token-major rows of ldq, or the head-major image
__device__ __forceinline__ int64_t ipa_q_at(const IpaArgs& a, int t, int h, int d) {
    return a.q_hstride ? (int64_t)h * a.q_hstride + (int64_t)t * d : (int64_t)t * a.ldq + h * d;
}

// softmax weights of the NT (>= N) scores in place, and scale / l
template <int NT>
__device__ __forceinline__ float ipa_softmax(float (&sc)[NT], int N, float scale) {
    float m = sc[0];
#pragma unroll
    for (int j = 1; j < NT; ++j)
        if (j < N) m = fmaxf(m, sc[j]);
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j)
        if (j < N) {
            sc[j] = __builtin_amdgcn_exp2f(sc[j] - m);
            l += sc[j];
        }
    return scale * (1.0f / l);
}

template <typename T>
__device__ __forceinline__ void ipa_stage(const IpaArgs& a, int b, int CV, typename Vec8<T>::type* ks, typename Vec8<T>::type* vs) {
    typedef typename Vec8<T>::type vec8;
    const T* kg = (const T*)a.k + (int64_t)b * a.N * a.ldkv;
    const T* vg = (const T*)a.v + (int64_t)b * a.N * a.ldkv;
    for (int i = threadIdx.x; i < a.N * CV; i += 256) {
        const int j = i / CV, c = i - j * CV;
        ks[i] = *reinterpret_cast<const vec8*>(kg + (int64_t)j * a.ldkv + c * 8);
        vs[i] = *reinterpret_cast<const vec8*>(vg + (int64_t)j * a.ldkv + c * 8);
    }
    __syncthreads();
}

// VPD = d / 8 vectors per head, NT = the unrolled bound on N (4 or 16)
template <typename T, int VPD, int NT>
__global__ void __launch_bounds__(256) ipa_kernel(const IpaArgs a) {
    typedef typename Vec8<T>::type vec8;
    extern __shared__ __attribute__((aligned(16))) unsigned char ipa_smem[];
    constexpr int D = VPD * 8, LANES = IpaGeom<VPD>::LANES, HPW = IpaGeom<VPD>::HPW, G = IpaGeom<VPD>::G, R = IpaGeom<VPD>::R;
    const int H = a.H, CV = H * VPD, C = H * D;
    vec8* ks = reinterpret_cast<vec8*>(ipa_smem);  // [N][CV]
    vec8* vs = ks + a.N * CV;                      // [N][CV]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)blockIdx.x / a.bps, blk = (int)blockIdx.x - b * a.bps;
    const bool lane_on = lane < LANES;
    const int hl = lane_on ? lane / VPD : 0, vv = lane_on ? lane - hl * VPD : 0, seg = hl * VPD;
    const T* qb = (const T*)a.q + a.q_off + (int64_t)b * a.T * a.ldq;
    T* ob = (T*)a.o + (int64_t)b * a.T * C;
    const int N = a.N;

    // one (token, head) pair group of this wave: its q and o vectors are requested one group ahead of their use (the first
    // before the keys and values are staged), so that a workgroup always has a group's loads in flight
    struct Item {
        vec8 q, o;
        T* op;
        int cv;
        bool on;
    };
    auto fetch = [&](int it) {
        Item m;
        m.q = vec8{};
        m.o = vec8{};
        const int pair = ((blk * a.iters + it) * 4 + wave) * HPW + hl;
        m.on = lane_on && it < a.iters && pair < a.pairs;
        const int t = pair / H, h = pair - t * H;
        m.op = ob + (int64_t)t * C + h * D + vv * 8;
        m.cv = h * VPD + vv;
        if (m.on) {
            m.q = *reinterpret_cast<const vec8*>(qb + ipa_q_at(a, t, h, D) + vv * 8);
            m.o = *reinterpret_cast<const vec8*>(m.op);
        }
        return m;
    };
    Item cur = fetch(0);
    ipa_stage<T>(a, b, CV, ks, vs);
    for (int it = 0; it < a.iters; ++it) {
        if (((blk * a.iters + it) * 4 + wave) * HPW >= a.pairs) break;  // wave-uniform
        const Item nxt = fetch(it + 1);
        float qf[8];
        ipa_unpack<T>(cur.q, qf);
        const int cv = cur.cv;
        float sc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            sc[j] = 0.f;
            if (j < N) {  // wave-uniform: every lane takes part in the lane exchanges
                float s = ipa_dot8<T>(qf, ks[j * CV + cv]);
#pragma unroll
                for (int m = 1; m < G; m <<= 1) s += __shfl_xor(s, m, 64);
                if constexpr (R > 1) {
                    float r = __shfl(s, seg, 64);
#pragma unroll
                    for (int i = 1; i < R; ++i) r += __shfl(s, seg + i * G, 64);
                    s = r;
                }
                sc[j] = s;
            }
        }
        const float w = ipa_softmax<NT>(sc, N, a.scale);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (j < N) {
                const vec8 vr = vs[j * CV + cv];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(sc[j], (float)vr[e], acc[e]);
            }
        if (cur.on) {
            vec8 res;
#pragma unroll
            for (int e = 0; e < 8; ++e) res[e] = (T)fmaf(acc[e], w, (float)cur.o[e]);
            *reinterpret_cast<vec8*>(cur.op) = res;
        }
        cur = nxt;
    }
}

// the alternative mapping: one thread per (token, head), same summation tree, same bits
template <typename T, int VPD, int NT>
__global__ void __launch_bounds__(256) ipa_kernel_per_head(const IpaArgs a) {
    typedef typename Vec8<T>::type vec8;
    extern __shared__ __attribute__((aligned(16))) unsigned char ipa_smem[];
    constexpr int D = VPD * 8, G = IpaGeom<VPD>::G, R = IpaGeom<VPD>::R;
    const int H = a.H, CV = H * VPD, C = H * D;
    vec8* ks = reinterpret_cast<vec8*>(ipa_smem);
    vec8* vs = ks + a.N * CV;
    const int tid = threadIdx.x;
    const int b = (int)blockIdx.x / a.bps, blk = (int)blockIdx.x - b * a.bps;
    ipa_stage<T>(a, b, CV, ks, vs);
    const T* qb = (const T*)a.q + a.q_off + (int64_t)b * a.T * a.ldq;
    T* ob = (T*)a.o + (int64_t)b * a.T * C;
    const int N = a.N;
    for (int it = 0; it < a.iters; ++it) {
        const int pair = (blk * a.iters + it) * 256 + tid;
        if (pair >= a.pairs) break;  // no barrier below
        const int t = pair / H, h = pair - t * H;
        const T* qp = qb + ipa_q_at(a, t, h, D);
        T* op = ob + (int64_t)t * C + h * D;
        vec8 qr[VPD];
#pragma unroll
        for (int i = 0; i < VPD; ++i) qr[i] = *reinterpret_cast<const vec8*>(qp + i * 8);
        float sc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            sc[j] = 0.f;
            if (j < N) {
                float pv[VPD];
#pragma unroll
                for (int i = 0; i < VPD; ++i) {
                    float qf[8];
                    ipa_unpack<T>(qr[i], qf);
                    pv[i] = ipa_dot8<T>(qf, ks[j * CV + h * VPD + i]);
                }
#pragma unroll
                for (int m = 1; m < G; m <<= 1)  // what the butterfly leaves in the first lane of every group of 2 m
#pragma unroll
                    for (int i = 0; i < VPD; i += 2 * m) pv[i] += pv[i + m];
                float s = pv[0];
#pragma unroll
                for (int i = 1; i < R; ++i) s += pv[i * G];
                sc[j] = s;
            }
        }
        const float w = ipa_softmax<NT>(sc, N, a.scale);
#pragma unroll
        for (int i = 0; i < VPD; ++i) {
            const vec8 orw = *reinterpret_cast<const vec8*>(op + i * 8);
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (j < N) {
                    const vec8 vr = vs[j * CV + h * VPD + i];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = fmaf(sc[j], (float)vr[e], acc[e]);
                }
            vec8 res;
#pragma unroll
            for (int e = 0; e < 8; ++e) res[e] = (T)fmaf(acc[e], w, (float)orw[e]);
            *reinterpret_cast<vec8*>(op + i * 8) = res;
        }
    }
}

constexpr int IPA_LDS_MAX = 2 * IPA_NMAX * IPA_CMAX * 2;  // 80 KB: N = 16, C = 1280

template <typename T, int VPD, int NT>
static int ipa_launch_one(const IpaArgs& a, int blocks, int lds, bool per_head, hipStream_t s) {
    if (per_head) {
        static std::atomic<uint64_t> done{0};
        set_lds_limit_once(done, reinterpret_cast<const void*>(&ipa_kernel_per_head<T, VPD, NT>), IPA_LDS_MAX);
        hipLaunchKernelGGL((ipa_kernel_per_head<T, VPD, NT>), dim3(blocks), dim3(256), lds, s, a);
    } else {
        static std::atomic<uint64_t> done{0};
        set_lds_limit_once(done, reinterpret_cast<const void*>(&ipa_kernel<T, VPD, NT>), IPA_LDS_MAX);
        hipLaunchKernelGGL((ipa_kernel<T, VPD, NT>), dim3(blocks), dim3(256), lds, s, a);
    }
    return last_error();
}

template <typename T>
static int ipa_launch(const IpaArgs& a, int d, int blocks, int lds, bool per_head, hipStream_t s) {
    const bool small = a.N <= 4;
#define IPA_CASE(VPD) \
    if (d == 8 * VPD) return small ? ipa_launch_one<T, VPD, 4>(a, blocks, lds, per_head, s) : ipa_launch_one<T, VPD, 16>(a, blocks, lds, per_head, s);
    IPA_CASE(4) IPA_CASE(5) IPA_CASE(8) IPA_CASE(10) IPA_CASE(16) IPA_CASE(20)
#undef IPA_CASE
    return UR_E_UNSUPPORTED;
}

}  // namespace ur

using namespace ur;

extern "C" int ur_ip_attention_add(void* o, const void* q, const void* k_ip, const void* v_ip, float scale, float qk_scale, int B,
                                   int H, int T, int d, int N, int64_t ldq, int q_off, int64_t q_hstride, int64_t ldkv, int flags,
                                   int dtype, void* stream) {
    if (!o || !q || !k_ip || !v_ip || B <= 0 || H <= 0 || T <= 0 || d <= 0 || N <= 0) return UR_E_BADARG;
    if (dtype != UR_DT_F16 && dtype != UR_DT_BF16) return UR_E_BADARG;
    if (!isfinite(scale) || (flags & ~(IPA_THREAD_PER_HEAD | (0xff << IPA_WALK_SHIFT)))) return UR_E_BADARG;
    if ((d != 32 && d != 40 && d != 64 && d != 80 && d != 128 && d != 160) || (int64_t)H * d > IPA_CMAX || N > IPA_NMAX) return UR_E_UNSUPPORTED;
    if (qk_scale > 0.f) return UR_E_UNSUPPORTED;  // the scores arrive in log2 units (q carries d^-1/2 log2 e), as the step's do
    const int64_t C = (int64_t)H * d;
    if (((uintptr_t)o | (uintptr_t)q | (uintptr_t)k_ip | (uintptr_t)v_ip) & 15) return UR_E_BADARG;
    if (q_off < 0 || (q_off & 7) || ldq <= 0 || (ldq & 7) || q_hstride < 0 || (q_hstride & 7) || ldkv < C || (ldkv & 7)) return UR_E_BADARG;
    if (q_hstride == 0 ? q_off + C > ldq : (q_hstride < (int64_t)T * d || q_off + (H - 1) * q_hstride + (int64_t)T * d > (int64_t)T * ldq))
        return UR_E_BADARG;
    if ((int64_t)T * H > (1 << 30)) return UR_E_UNSUPPORTED;
    if (scale == 0.f) return 0;  // o + 0 * ip: nothing to do, and o keeps its bits
    const bool per_head = (flags & IPA_THREAD_PER_HEAD) != 0;
    IpaArgs a{};
    a.o = o; a.q = q; a.k = k_ip; a.v = v_ip;
    a.scale = scale; a.T = T; a.N = N; a.H = H; a.pairs = T * H; a.q_off = q_off;
    a.ldq = ldq; a.q_hstride = q_hstride; a.ldkv = ldkv;
    // a workgroup stages its sample's 4 N C bytes (out of L2) once and then walks `iters` groups of (token, head) pairs.  While
    // the launch has fewer than two workgroups per CU, every group gets its own workgroup -- the deep levels are a few hundred
    // groups and a serial walk only adds latency (measured: DESIGN.md) -- beyond that the walk grows with the launch, up to 16
    const int per_iter = per_head ? 256 : 4 * (64 / (d / 8));
    const int64_t groups = ((int64_t)a.pairs + per_iter - 1) / per_iter;
    int64_t iters = groups * B / IPA_GROUPS_PER_WALK;
    iters = iters < 1 ? 1 : (iters > 16 ? 16 : iters);
    if ((flags >> IPA_WALK_SHIFT) & 0xff) iters = (flags >> IPA_WALK_SHIFT) & 0xff;  // A/B runs, tests
    if (iters > groups) iters = groups;
    a.iters = (int)iters;
    a.bps = (int)((groups + iters - 1) / iters);
    const int64_t blocks = (int64_t)B * a.bps;
    if (blocks > (1 << 30)) return UR_E_UNSUPPORTED;
    const int lds = (int)(2 * N * C * 2);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    UR_DISPATCH(dtype, return ipa_launch<T>(a, d, (int)blocks, lds, per_head, st));
}
