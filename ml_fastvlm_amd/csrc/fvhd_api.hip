// C ABI (include/fvhd.h): context, weight packing, workspace and the launch sequence of the
// FastViTHD encode_images() path.  The sequence below is the reference's
// FastViT.forward (mci.py:1427-1451) with every module replaced by its gfx950 kernel; the block
// structure follows fastvithd() (mci.py:1454-1478).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "api_host.h"
#include "launchers.h"

namespace {

thread_local std::string g_err;

int fail(const std::string& msg, int code = 1)
{
    g_err = msg;
    return code ? code : 1;
}

int hip_fail(const char* what, hipError_t e)
{
    return fail(std::string(what) + ": " + hipGetErrorString(e), (int)e ? (int)e : 1);
}

// fastvithd() hyper-parameters, mci.py:1455-1460
constexpr int kStages = 5;
constexpr int kLayers[kStages] = {2, 12, 24, 4, 2};
constexpr int kDims[kStages] = {96, 192, 384, 768, 1536};
constexpr int kOutDim = 3072;   // cls_ratio 2.0 * 1536 (mci.py:1403)
constexpr int kSeRd = 192;      // 3072 * 0.0625 (mci.py:49)
constexpr float kBnEps = 1e-5f, kLnEps = 1e-5f;

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

struct Packer {          // builds the packed weight image on the host; offsets are 256-B aligned
    std::vector<char> buf;
    size_t reserve(size_t bytes)
    {
        size_t off = (buf.size() + 255) & ~(size_t)255;
        buf.resize(off + bytes);
        return off;
    }
    size_t add_f32(const float* p, size_t n)
    {
        size_t off = reserve(n * 4);
        memcpy(buf.data() + off, p, n * 4);
        return off;
    }
    size_t add_bf16(const float* p, size_t n)
    {
        size_t off = reserve(n * 2);
        uint16_t* d = (uint16_t*)(buf.data() + off);
        for (size_t i = 0; i < n; ++i) d[i] = f32_to_bf16_rne(p[i]);
        return off;
    }
};

struct DwW { size_t w = 0, b = 0; int K = 0; bool bf16_taps = false; };   // taps fp32 [K*K][Cout], bias fp32 [Cout]; bf16_taps: every packed tap is a bf16 number
struct GemmW { size_t w = 0, b = 0; int N = 0, K = 0; bool has_bias = false; };
// w?img: chunk images of the fused kernel in its two precisions ([0] FVHD_FFN_HALF: W1 / 4 in bf16, 4 W2 in f16; [1] FVHD_FFN_BF16);
// precision: which one this block runs (fvhd_set_ffn_precision / fvhd_audit_ranges; FVHD_FFN_BF16 from the start if |4 W2| would overflow f16)
// guard_limit (round 5): the largest max |A| (A = the dw7x7 + BN output the block's fc1 reads) for which the half-precision form is PROVABLY in
// range: |fc1 out_j| <= sum_c |W1[j][c]| max|A| + |b1_j|, so max_j L1(W1 row j) * max|A| + max_j |b1_j| <= kGuardFc1Limit keeps every hidden
// pre-activation at least a factor 2 below the 262 016 where gelu(x) / 4 saturates in IEEE half (the range guard, fvhd.h)
struct FfnW { DwW dw7; GemmW fc1, fc2; size_t ls = 0; size_t w1img[2] = {0, 0}, w2img[2] = {0, 0}; bool fused = false; int precision = FVHD_FFN_HALF;
              float guard_limit = 0.f, guard_limit_y = 0.f; };
// guard_limit_y: the same guarantee one convolution earlier - a limit on max |y| of the block's dw7x7 INPUT (= the RepMixer output), through
// |A_c| <= L1(folded 7x7 taps of channel c) max|y| + |folded bias_c|: looser by the taps' L1 norm, but max |y| can be reduced inside the
// HBM-bound 3x3 kernel instead of the matrix-core 7x7 (FVHD_GUARD_SITE, fvhd.h "range guard")
struct RepBlockW { DwW mixer; FfnW ffn; };
struct AttnBlockW { size_t ln_w = 0, ln_b = 0, ls1 = 0; GemmW qkv, proj; FfnW ffn; };
struct DownW { DwW dw; GemmW pw; };

// One "step" = one forward() of a reference module on the running activation (execution order of
// FastViT.forward, mci.py:1427-1451): stem, then per stage [RepCPE], blocks, [PatchEmbed], then conv_exp+SE.
enum StepKind { S_STEM, S_CPE, S_REP, S_ATT, S_DOWN, S_HEAD };
struct Step { int kind, stage, idx, C, hdiv, Cout, hdiv_out; };   // H = R / hdiv on entry, R / hdiv_out on exit

struct Model {
    std::vector<Step> steps;
    size_t stem0_w = 0, stem0_b = 0;
    DwW stem1;
    GemmW stem2;
    std::vector<RepBlockW> rep[3];
    std::vector<AttnBlockW> att[2];
    DownW down[4];
    DwW cpe[2];
    DwW conv_exp;
    size_t se_wr = 0, se_br = 0, se_we = 0, se_be = 0;
};

struct ProfRec { int cls; hipEvent_t a, b; };
#ifndef FVHD_GUARD_SITE_DEFAULT
#define FVHD_GUARD_SITE_DEFAULT 0      // the tighter bound; both sites cost < 0.3 % of the step since the slot fix (profiles/r05_guard_cost_ab.log)
#endif
constexpr float kGuardFc1Limit = 131072.0f;      // 2^17: half of the f16 saturation point of the fused kernel's hidden pre-activation
constexpr int kGuardSlots = 4;                   // read-backs of the range guard in flight (one per encode call)
constexpr int kAmaxSlots = 64;                   // = FVHD_AMAX_SLOTS of csrc/fvhd_common.h: words per step the kernels spread their atomics over
struct GuardSlot { unsigned* host = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
struct GuardHit { int step; float amax; };

const char* kClassNames[] = {"stem", "dw3", "dw7", "dw_down", "gemm_fc1", "gemm_fc2", "gemm_1x1", "gemm_qkv",
                             "gemm_proj", "layernorm", "attention", "head", "projector", "ffn_fused", "dw_mix"};
enum { C_STEM, C_DW3, C_DW7, C_DWDOWN, C_FC1, C_FC2, C_1X1, C_QKV, C_PROJ, C_LN, C_ATT, C_HEAD, C_PROJECTOR, C_FFN, C_DWMIX, C_COUNT };

}  // namespace

struct fvhd_ctx {
    int device = 0, R = 0, max_batch = 0;
    std::map<std::string, HostTensor> raw;
    Model m;
    char* wdev = nullptr;
    bool finalized = false;
    // projector
    char* pdev = nullptr;
    GemmW p0, p2;
    int mm_hidden = 0, hidden = 0;
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    int ws_batch = 0, ws_hidden = 0;
    // A call that ran while ITS CALLER was capturing the stream put this arena's pointers into the caller's graph.  Such an arena is never
    // freed when a later call needs a bigger one: it is retired (kept until fvhd_destroy), so the captured graph keeps replaying on valid
    // memory (round 5: what the LLM workspace has done since round 4 - VERDICT r4 weak #9)
    bool ws_captured = false;
    std::vector<char*> ws_retired;
    bool use_fused_ffn = true;   // FVHD_FUSED_FFN=0 falls back to fc1 / fc2 as two GEMM launches (A/B measurements)
    bool use_fused_dw = true;    // FVHD_FUSED_DW=0: RepMixer dw3x3 and ConvFFN dw7x7 always as two launches (A/B measurements)
    bool use_splitk = true;      // FVHD_GEMM_SPLITK=0: never split the K of the residual GEMMs (A/B measurements)
    // FVHD_FUSED_STEM: 2 (default) the whole convolutional_stem in ONE launch; 1: stem[0] + stem[1] fused, stem[2] as a GEMM launch (rounds
    // 1-3); 0: three launches through a [B,R/2,R/2,96] HBM tensor.  All three give the same bits.
    int use_fused_stem = 2;
    int attn_fp8 = 0;            // fvhd_set_attention_fp8 / FVHD_ATTN_FP8=1: e4m3 MFMA operands in MHSA (BASELINE.json configs[4]; opt-in)
    int batch_invariant = 0;     // fvhd_set_batch_invariant: kernel choice by image shape only (bit-identical rows in any batch)
    // fvhd_audit_ranges: while set, every ConvFFN also runs its fc1 as a plain GEMM (bias, no GELU) and reduces max |fc1 out| into
    // audit_dev[step] (fp32 bit patterns of non-negative values, ordered as unsigned integers)
    unsigned* audit_dev = nullptr;
    // range guard (round 5; fvhd.h "range guard"): every dw7x7 that feeds a half-precision fused ConvFFN reduces max |A| into guard_dev[step]
    // (zeroed per encode call); the array is read back asynchronously and compared with FfnW::guard_limit when the NEXT call polls it
    int guard_on = 1;
    int guard_site = FVHD_GUARD_SITE_DEFAULT;    // 0: max |A| inside the dw7x7 (+BN) kernels, 1: max |y| inside the RepMixer dw3x3 kernel
    unsigned* guard_dev = nullptr;
    int guard_n = 0, guard_next = 0;
    GuardSlot guard_slots[kGuardSlots];
    std::vector<GuardHit> guard_hits;           // switched since the last fvhd_range_guard_poll
    bool guard_active = false;                   // this call's launches carry the amax pointers
    // hipGraph replay of the interior steps (fvhd_set_graph / FVHD_GRAPH=1): ~170 launches become one hipGraphLaunch.
    // The stem (reads the caller's images) and the head (writes the caller's buffer) stay outside the graph, so a cached
    // graph only holds library-owned pointers (workspace, packed weights) and is valid for any caller buffers.
    struct GraphEntry {
        int B, fused;              // fused: bit 0 fused ConvFFN, bit 1 batch-invariant dispatch, bit 2 e4m3 attention operands
        char* ws;
        hipGraphExec_t exec;       // nullptr until the second call with this key (the first runs eagerly), or when capture failed
        bool failed;
        char *X, *T;               // activation ping-pong state after the interior steps
    };
    int graph = 0;
    std::vector<GraphEntry> graphs;
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> ev_pool;
    double acc_ms[C_COUNT] = {0};
    int64_t acc_n[C_COUNT] = {0};

    template <typename T> const T* wp(size_t off) const { return (const T*)(wdev + off); }
};

namespace {

const HostTensor* find(const fvhd_ctx* c, const std::string& key, std::initializer_list<int64_t> shape)
{
    auto it = c->raw.find(key);
    if (it == c->raw.end()) { fail("missing tensor: " + key); return nullptr; }
    size_t i = 0;
    bool ok = it->second.shape.size() == shape.size();
    if (ok) for (int64_t s : shape) ok = ok && (it->second.shape[i++] == s);
    if (!ok) { fail("bad shape for tensor: " + key); return nullptr; }
    return &it->second;
}

// depthwise taps [Cout,1,K,K] -> fp32 [K*K][Cout] (optionally scaled per channel), bias [Cout]
bool pack_dw(fvhd_ctx* c, Packer& pk, const std::string& wkey, const std::string& bkey, int Cout, int K, DwW* out,
             const std::vector<float>* ch_scale = nullptr, const std::vector<float>* ch_bias = nullptr)
{
    const HostTensor* w = find(c, wkey, {Cout, 1, K, K});
    if (!w) return false;
    std::vector<float> t((size_t)K * K * Cout), b((size_t)Cout, 0.f);
    for (int oc = 0; oc < Cout; ++oc) {
        const float s = ch_scale ? (*ch_scale)[oc] : 1.0f;
        for (int k = 0; k < K * K; ++k) t[(size_t)k * Cout + oc] = w->data[(size_t)oc * K * K + k] * s;
    }
    if (!bkey.empty()) {
        const HostTensor* bt = find(c, bkey, {Cout});
        if (!bt) return false;
        b = bt->data;
    }
    if (ch_bias) b = *ch_bias;
    out->w = pk.add_f32(t.data(), t.size());
    out->b = pk.add_f32(b.data(), b.size());
    out->K = K;
    out->bf16_taps = true;                   // (a bf16 tower with re-parameterised convolutions: the taps a matrix-core kernel rounds to are the taps)
    for (float v : t) {
        uint32_t u;
        memcpy(&u, &v, 4);
        if (u & 0xffffu) { out->bf16_taps = false; break; }
    }
    return true;
}

bool pack_gemm(fvhd_ctx* c, Packer& pk, const std::string& wkey, const std::string& bkey, int N, int K, bool conv,
               GemmW* out)
{
    const HostTensor* w = conv ? find(c, wkey, {N, K, 1, 1}) : find(c, wkey, {N, K});
    if (!w) return false;
    out->w = pk.add_bf16(w->data.data(), (size_t)N * K);
    out->N = N;
    out->K = K;
    out->has_bias = !bkey.empty();
    if (out->has_bias) {
        const HostTensor* b = find(c, bkey, {N});
        if (!b) return false;
        out->b = pk.add_f32(b->data.data(), N);
    }
    return true;
}

bool pack_vec(fvhd_ctx* c, Packer& pk, const std::string& key, std::initializer_list<int64_t> shape, size_t* off)
{
    const HostTensor* t = find(c, key, shape);
    if (!t) return false;
    *off = pk.add_f32(t->data.data(), t->data.size());
    return true;
}

// ConvFFN (mci.py:862-927): dw7x7 (no bias) + eval BatchNorm folded into taps/bias, fc1, fc2; layer scale key given
bool pack_ffn(fvhd_ctx* c, Packer& pk, const std::string& p, const std::string& ls_key, int C, FfnW* out)
{
    const HostTensor* g = find(c, p + ".convffn.conv.bn.weight", {C});
    const HostTensor* be = find(c, p + ".convffn.conv.bn.bias", {C});
    const HostTensor* mu = find(c, p + ".convffn.conv.bn.running_mean", {C});
    const HostTensor* var = find(c, p + ".convffn.conv.bn.running_var", {C});
    if (!g || !be || !mu || !var) return false;
    // y = (conv - mu) / sqrt(var + eps) * gamma + beta  =>  w' = w * s, b' = beta - mu * s, s = gamma / sqrt(var + eps)
    std::vector<float> s(C), b(C);
    for (int i = 0; i < C; ++i) {
        s[i] = g->data[i] / sqrtf(var->data[i] + kBnEps);
        b[i] = be->data[i] - mu->data[i] * s[i];
    }
    if (!pack_dw(c, pk, p + ".convffn.conv.conv.weight", "", C, 7, &out->dw7, &s, &b)) return false;
    if (!pack_gemm(c, pk, p + ".convffn.fc1.weight", p + ".convffn.fc1.bias", 4 * C, C, true, &out->fc1)) return false;
    if (!pack_gemm(c, pk, p + ".convffn.fc2.weight", p + ".convffn.fc2.bias", C, 4 * C, true, &out->fc2)) return false;
    // chunk images for the fused MLP kernel (ffn_fused.hip: fvhd_ffn_pack_host)
    if (fvhd_ffn_fused_supported(C)) {
        const HostTensor* w1 = find(c, p + ".convffn.fc1.weight", {4 * C, C, 1, 1});
        const HostTensor* w2 = find(c, p + ".convffn.fc2.weight", {C, 4 * C, 1, 1});
        if (!w1 || !w2) return false;
        const size_t che = (size_t)32 * C, nch = (size_t)4 * C / 32;
        for (int pr = 0; pr < 2; ++pr) {
            out->w1img[pr] = pk.reserve((nch + 1) * che * 2);
            out->w2img[pr] = pk.reserve(nch * che * 2);     // (reserve may move buf: take the pointers after both calls)
            if (fvhd_ffn_pack_host(C, w1->data.data(), w2->data.data(), (uint16_t*)(pk.buf.data() + out->w1img[pr]),
                                   (uint16_t*)(pk.buf.data() + out->w2img[pr]), pr)) return false;
        }
        float w2max = 0.f;
        for (float v : w2->data) w2max = fmaxf(w2max, fabsf(v));
        // f16(4 W2) must stay finite - and must not sink into the f16 subnormals (|4 W2| < 6.1e-5 carries fewer than 11 bits): a block whose
        // LARGEST fc2 weight is below 2^-10 would lose most of its weights' precision on the half form (real checkpoints: 1e-2 .. 1e-1)
        out->precision = (w2max < fvhd_ffn_half_w2_limit() && w2max >= 0.0009765625f) ? FVHD_FFN_HALF : FVHD_FFN_BF16;
        // range guard: L1 norms of the fc1 rows as the kernel sees them (bf16-rounded weights), largest |bias|
        const HostTensor* b1 = find(c, p + ".convffn.fc1.bias", {4 * C});
        if (!b1) return false;
        double l1max = 0.0, b1max = 0.0;
        bool finite = true;
        for (int j = 0; j < 4 * C; ++j) {
            double l1 = 0.0;
            for (int k = 0; k < C; ++k) {
                const uint32_t u = (uint32_t)f32_to_bf16_rne(w1->data[(size_t)j * C + k]) << 16;
                float r;
                memcpy(&r, &u, 4);
                l1 += fabs((double)r);
            }
            finite = finite && std::isfinite(l1) && std::isfinite(b1->data[j]);
            l1max = l1 > l1max ? l1 : l1max;
            b1max = fabs((double)b1->data[j]) > b1max ? fabs((double)b1->data[j]) : b1max;
        }
        // (a 1 % allowance for the rounding of A to bf16 and of the fp32 accumulation is part of the factor 2 in kGuardFc1Limit)
        out->guard_limit = (!finite || b1max >= kGuardFc1Limit) ? -1.f : (l1max > 0.0 ? (float)((kGuardFc1Limit - b1max) / l1max) : INFINITY);
        if (out->guard_limit < 0.f) out->precision = FVHD_FFN_BF16;       // the biases alone leave the half-precision range: never on that form
        // one convolution earlier: folded 7x7 taps w'[c][k] = w[c][k] s[c] and bias b'[c] (the values pack_dw uploads)
        const HostTensor* w7 = find(c, p + ".convffn.conv.conv.weight", {C, 1, 7, 7});
        if (!w7) return false;
        double t7max = 0.0, b7max = 0.0;
        for (int ch = 0; ch < C; ++ch) {
            double l1 = 0.0;
            for (int k = 0; k < 49; ++k) l1 += fabs((double)(w7->data[(size_t)ch * 49 + k] * s[ch]));
            finite = finite && std::isfinite(l1) && std::isfinite(b[ch]);
            t7max = l1 > t7max ? l1 : t7max;
            b7max = fabs((double)b[ch]) > b7max ? fabs((double)b[ch]) : b7max;
        }
        if (out->guard_limit < 0.f || !finite) out->guard_limit_y = -1.f;
        else if (!(out->guard_limit < INFINITY) || t7max == 0.0) out->guard_limit_y = (b7max <= out->guard_limit) ? INFINITY : 0.f;
        else out->guard_limit_y = (float)fmax(0.0, ((double)out->guard_limit - b7max) / t7max);
        out->fused = true;
    }
    return pack_vec(c, pk, ls_key, {C, 1, 1}, &out->ls);
}

#define FVHD_ON_DEVICE(c)                                              \
    DeviceGuard _guard((c)->device);                                   \
    if (_guard.err != hipSuccess) return hip_fail("hipSetDevice", _guard.err)

constexpr size_t kSplitKPartialBytes = (size_t)512 * 128 * 128 * 4;   // fvhd_gemm_splitk_plan: at most 512 (tile, slice) pairs of 128 x 128 fp32

struct Ws {   // workspace carve-up for batch B
    char *X, *T, *A, *H, *tok, *ph, *cast;
    float *pooled, *scale, *part;                                    // part: fp32 partial sums of the split-K residual GEMMs (small batches)
    size_t total;
};

Ws carve(const fvhd_ctx* c, char* base, int B, int hidden)
{
    const size_t unit = (size_t)(c->R / 4) * (c->R / 4) * 96 * 2 * B;   // bytes of one stage-0 activation (bf16)
    const size_t Tn = (size_t)(c->R / 64) * (c->R / 64);
    Ws w;
    Arena a;
    auto take = [&](size_t bytes) { const size_t o = a.take(bytes); return base ? base + o : nullptr; };
    w.X = take(unit);
    w.T = take(unit);
    w.A = take(unit);
    w.H = take(4 * unit);
    w.tok = take(Tn * B * kOutDim * 2);
    w.ph = take(Tn * B * (size_t)(hidden > 0 ? hidden : 1) * 2);
    w.cast = take(Tn * B * kOutDim * 2);
    w.pooled = (float*)take((size_t)B * (kOutDim + kSeRd) * 4);
    w.scale = (float*)take((size_t)B * kOutDim * 4);
    w.part = (float*)take(kSplitKPartialBytes);
    w.total = a.off;
    return w;
}

void clear_graphs(fvhd_ctx* c)
{
    for (auto& g : c->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    c->graphs.clear();
}

// Growing the arena synchronises the device, frees and re-allocates: never legal while `st` is being captured into a graph
// (the caller must fvhd_reserve() the batch size before it starts capturing).
int ensure_ws(fvhd_ctx* c, int B, hipStream_t st = nullptr, bool check_capture = false)
{
    if (c->ws && B <= c->ws_batch && c->hidden <= c->ws_hidden) return 0;
    if (check_capture && is_capturing(st))
        return fail("fvhd: the workspace must grow for this batch size but the stream is being captured - call fvhd_reserve(ctx, batch) before capturing");
    clear_graphs(c);                         // cached graphs point into the old arena
    const int nb = B > c->ws_batch ? B : c->ws_batch;
    const size_t need = carve(c, nullptr, nb, c->hidden).total;
    hipError_t e = hipDeviceSynchronize();   // growing the arena: make sure nothing still uses the old one
    if (e != hipSuccess) return hip_fail("hipDeviceSynchronize", e);
    if (c->ws) {
        if (c->ws_captured) c->ws_retired.push_back(c->ws);   // a caller's graph still points into it
        else (void)hipFree(c->ws);
    }
    c->ws = nullptr;
    c->ws_captured = false;
    e = hipMalloc((void**)&c->ws, need);
    if (e != hipSuccess) return hip_fail("hipMalloc(workspace)", e);
    c->ws_bytes = need;
    c->ws_batch = nb;
    c->ws_hidden = c->hidden;
    return 0;
}

hipEvent_t get_event(fvhd_ctx* c)
{
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

struct Scope {   // brackets one launch with events when profiling is on
    fvhd_ctx* c; hipStream_t st; int idx = -1;
    Scope(fvhd_ctx* c_, hipStream_t st_, int cls) : c(c_), st(st_)
    {
        if (!c->prof) return;
        ProfRec r{cls, get_event(c), get_event(c)};
        (void)hipEventRecord(r.a, st);
        c->recs.push_back(r);
        idx = (int)c->recs.size() - 1;
    }
    ~Scope() { if (idx >= 0) (void)hipEventRecord(c->recs[idx].b, st); }
};

#define CHECK_LAUNCH(expr, what)                                              \
    do {                                                                      \
        int _e = (expr);                                                      \
        if (_e) return hip_fail(what, (hipError_t)_e);                        \
    } while (0)

// max |x| over n8 * 8 bf16 values, as the fp32 bit pattern of a non-negative number (unsigned order = numeric order; Inf and NaN sort
// above every finite value, so an overflow anywhere in the tensor surfaces in the result)
__global__ __launch_bounds__(256) void absmax_bf16_kernel(const uint16_t* __restrict__ x, long n8, unsigned* __restrict__ out)
{
    unsigned m = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const uint4 v = *(const uint4*)(x + i * 8);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned lo = w[k] & 0x7fffu, hi = (w[k] >> 16) & 0x7fffu;
            m = m > lo ? m : lo;
            m = m > hi ? m : hi;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
        m = m > o ? m : o;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m << 16);
}

FfnW* ffn_of_step(fvhd_ctx* c, int step)
{
    if (!c || !c->finalized || step < 0 || step >= (int)c->m.steps.size()) return nullptr;
    const Step& sp = c->m.steps[step];
    if (sp.kind == S_REP) return &c->m.rep[sp.stage][sp.idx].ffn;
    if (sp.kind == S_ATT) return &c->m.att[sp.stage - 3][sp.idx].ffn;
    return nullptr;
}

// ---- range guard of the half-precision fused ConvFFN (include/fvhd.h "range guard") -----------------------------------------------
void guard_free(fvhd_ctx* c)
{
    for (auto& sl : c->guard_slots) {
        if (sl.pending && sl.ev) (void)hipEventSynchronize(sl.ev);
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.ev) (void)hipEventDestroy(sl.ev);
        sl = GuardSlot();
    }
    if (c->guard_dev) (void)hipFree(c->guard_dev);
    c->guard_dev = nullptr;
    c->guard_n = 0;
    c->guard_next = 0;
}

int guard_alloc(fvhd_ctx* c, int n)
{
    guard_free(c);
    const size_t bytes = (size_t)n * kAmaxSlots * 4;
    hipError_t e = hipMalloc((void**)&c->guard_dev, bytes);
    if (e != hipSuccess) return hip_fail("hipMalloc(range guard)", e);
    e = hipMemset(c->guard_dev, 0, bytes);
    for (auto& sl : c->guard_slots) {
        if (e == hipSuccess) e = hipHostMalloc((void**)&sl.host, bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming);
    }
    if (e != hipSuccess) { guard_free(c); return hip_fail("range guard allocation", e); }
    c->guard_n = n;
    return 0;
}

// one finished read-back against the per-block limits: a block whose bound is exceeded moves to the bf16-operand form for every later call
bool guard_check_slot(fvhd_ctx* c, const GuardSlot& sl)
{
    bool switched = false;
    for (int i = 0; i < c->guard_n; ++i) {
        FfnW* f = ffn_of_step(c, i);
        if (!f || !f->fused || f->precision != FVHD_FFN_HALF) continue;
        unsigned bits = 0;                          // maximum of the step's row (bit patterns of non-negative floats: unsigned order)
        for (int k = 0; k < kAmaxSlots; ++k) bits = sl.host[(size_t)i * kAmaxSlots + k] > bits ? sl.host[(size_t)i * kAmaxSlots + k] : bits;
        float a;
        memcpy(&a, &bits, 4);
        // (+Inf sorts above every finite value and trips the guard.  A NaN in A does NOT: the kernels reduce with fmaxf, which drops NaN
        // operands - a NaN activation reaches the output on either form of the block, the guard is about finite overflow only.)
        if (!(a <= (c->guard_site == 1 ? f->guard_limit_y : f->guard_limit))) {
            f->precision = FVHD_FFN_BF16;
            c->guard_hits.push_back(GuardHit{i, a});
            switched = true;
        }
    }
    return switched;
}

// consume the read-backs that have finished (all of them when wait); returns the number of blocks switched by this call
int guard_process(fvhd_ctx* c, bool wait)
{
    bool switched = false;
    for (auto& sl : c->guard_slots) {
        if (!sl.pending) continue;
        const hipError_t q = wait ? hipEventSynchronize(sl.ev) : hipEventQuery(sl.ev);
        if (q == hipErrorNotReady) continue;
        sl.pending = false;
        if (q != hipSuccess) { (void)hipGetLastError(); continue; }
        switched = guard_check_slot(c, sl) || switched;
    }
    if (switched) {
        (void)hipDeviceSynchronize();            // cached graphs hold the other kernel and the other weight images
        clear_graphs(c);
    }
    return switched ? 1 : 0;
}

int run_dw(fvhd_ctx* c, hipStream_t st, int cls, const DwW& w, const void* x, void* y, int B, int H, int W, int Cin,
           int stride, int mult, int gelu, unsigned* amax = nullptr)
{
    Scope s(c, st, cls);
    CHECK_LAUNCH(fvhd_launch_dwconv(st, x, y, c->wp<float>(w.w), c->wp<float>(w.b), B, H, W, Cin, w.K, stride, mult, gelu,
                                    (c->batch_invariant ? 1 : 0) | (w.bf16_taps ? 0 : 2), amax),
                 "dwconv launch");
    return 0;
}

int run_gemm(fvhd_ctx* c, hipStream_t st, int cls, const char* wbase, const GemmW& g, const void* A, const float* ls,
             const void* resid, void* out, int M, int epi, int odt = FVHD_BF16, float* part = nullptr)
{
    Scope s(c, st, cls);
    // residual GEMMs with a handful of output tiles and a long K (fc2 / proj at B = 1-8): K split across workgroups.  Not in batch-invariant
    // mode: the number of slices - the summation order - depends on the batch
    if (part && epi == FVHD_EPI_BIAS_LS_RESID && odt == FVHD_BF16 && g.has_bias && c->use_splitk && !c->batch_invariant) {
        const int sp = fvhd_gemm_splitk_plan(M, g.N, g.K);
        if (sp > 1) {
            CHECK_LAUNCH(fvhd_launch_gemm_splitk_ls(st, A, wbase + g.w, (const float*)(wbase + g.b), ls, resid, out, part, M, g.N, g.K, sp),
                         "split-K gemm launch");
            return 0;
        }
    }
    CHECK_LAUNCH(fvhd_launch_gemm(st, A, wbase + g.w, g.has_bias ? (const float*)(wbase + g.b) : nullptr, ls, resid, out,
                                  M, g.N, g.K, epi, odt),
                 "gemm launch");
    return 0;
}

constexpr int kFusedFfnMinRows = 24576;

// ConvFFN + layer scale + residual, in place on x (mci.py:1106-1109 / 1185-1188 second line)
bool ffn_takes_fused(const fvhd_ctx* c, const FfnW& f, int M) { return f.fused && c->use_fused_ffn && (c->batch_invariant || M >= kFusedFfnMinRows); }

// range guard, site 0: the depthwise conv that feeds a half-precision fused block also reduces max |A| into this step's slot
unsigned* ffn_amax_slot(fvhd_ctx* c, const FfnW& f, int M, int step)
{
    return (c->guard_active && c->guard_site == 0 && ffn_takes_fused(c, f, M) && f.precision == FVHD_FFN_HALF && step < c->guard_n)
               ? c->guard_dev + (size_t)step * kAmaxSlots : nullptr;
}

// have_a: w.A already holds dw7x7(x) + BN (the RepMixerBlock's one-launch dw3x3 -> dw7x7, run_step)
int run_ffn(fvhd_ctx* c, hipStream_t st, const FfnW& f, const Ws& w, char* x, int B, int H, int Wd, int C, int step, bool have_a = false)
{
    const int M = B * H * Wd;
    int e;
    const bool take_fused = ffn_takes_fused(c, f, M);
    if (!have_a && (e = run_dw(c, st, C_DW7, f.dw7, x, w.A, B, H, Wd, C, 1, 1, 0, ffn_amax_slot(c, f, M, step)))) return e;
    if (c->audit_dev) {          // range audit: fc1 + bias as a plain GEMM into the hidden buffer, max |.| of it into this step's slot
        if ((e = run_gemm(c, st, C_FC1, c->wdev, f.fc1, w.A, nullptr, nullptr, w.H, M, FVHD_EPI_BIAS))) return e;
        const long n8 = (long)M * 4 * C / 8;
        hipLaunchKernelGGL(absmax_bf16_kernel, dim3((unsigned)((n8 + 255) / 256 < 4096 ? (n8 + 255) / 256 : 4096)), dim3(256), 0, st,
                           (const uint16_t*)w.H, n8, c->audit_dev + step);
        CHECK_LAUNCH((int)hipGetLastError(), "absmax launch");
    }
    // The fused kernel gives one workgroup 128 rows and walks the whole hidden dimension serially (48 chunks at C = 384: ~60 us
    // however few rows there are).  Below ~0.75 workgroups per CU the two tiled GEMMs (hundreds of tiles even at M = 4096) finish
    // sooner: B = 1 at 1024^2 runs stages 2 / 3 (M = 16384 / 4096) this way, 4.27 -> 3.4 ms per image.
    if (take_fused) {
        Scope s(c, st, C_FFN);
        CHECK_LAUNCH(fvhd_launch_ffn_fused(st, w.A, c->wdev + f.w1img[f.precision], c->wp<float>(f.fc1.b), c->wdev + f.w2img[f.precision],
                                           c->wp<float>(f.fc2.b), c->wp<float>(f.ls), x, M, C, f.precision),
                     "fused ffn launch");
        return 0;
    }
    if ((e = run_gemm(c, st, C_FC1, c->wdev, f.fc1, w.A, nullptr, nullptr, w.H, M, FVHD_EPI_BIAS_GELU))) return e;
    return run_gemm(c, st, C_FC2, c->wdev, f.fc2, w.H, c->wp<float>(f.ls), x, x, M, FVHD_EPI_BIAS_LS_RESID, FVHD_BF16, w.part);
}

int run_step(fvhd_ctx* c, hipStream_t st, const Step& sp, const Ws& w, char*& X, char*& T, int B, const void* images,
             int img_dtype, void* out, int out_dtype)
{
    const Model& m = c->m;
    const int R = c->R, H = R / sp.hdiv, C = sp.C, M = B * H * H;
    int e;
    switch (sp.kind) {
    case S_STEM: {   // convolutional_stem (mci.py:553-603)
        if (c->use_fused_stem == 2) {
            Scope s(c, st, C_STEM);
            CHECK_LAUNCH(fvhd_launch_stem_fused(st, images, img_dtype, X, c->wp<float>(m.stem0_w), c->wp<float>(m.stem0_b),
                                                c->wp<float>(m.stem1.w), c->wp<float>(m.stem1.b), c->wdev + m.stem2.w, c->wp<float>(m.stem2.b), B, R),
                         "fused stem launch");
            return 0;
        }
        if (c->use_fused_stem) {
            {
                Scope s(c, st, C_STEM);
                CHECK_LAUNCH(fvhd_launch_stem_fused(st, images, img_dtype, w.A, c->wp<float>(m.stem0_w), c->wp<float>(m.stem0_b),
                                                    c->wp<float>(m.stem1.w), c->wp<float>(m.stem1.b), nullptr, nullptr, B, R),
                             "fused stem launch");
            }
            return run_gemm(c, st, C_STEM, c->wdev, m.stem2, w.A, nullptr, nullptr, X, B * (R / 4) * (R / 4), FVHD_EPI_BIAS_GELU);
        }
        {
            Scope s(c, st, C_STEM);
            CHECK_LAUNCH(fvhd_launch_stem_conv(st, images, img_dtype, w.H, c->wp<float>(m.stem0_w), c->wp<float>(m.stem0_b), B, R),
                         "stem conv launch");
        }
        if ((e = run_dw(c, st, C_STEM, m.stem1, w.H, w.A, B, R / 2, R / 2, 96, 2, 1, 1))) return e;
        return run_gemm(c, st, C_STEM, c->wdev, m.stem2, w.A, nullptr, nullptr, X, B * (R / 4) * (R / 4), FVHD_EPI_BIAS_GELU);
    }
    case S_CPE:      // RepCPE (mci.py:992-995)
        if ((e = run_dw(c, st, C_DW7, m.cpe[sp.stage - 3], X, T, B, H, H, C, 1, 1, 0))) return e;
        std::swap(X, T);
        return 0;
    case S_REP: {    // RepMixerBlock (mci.py:1106-1109)
        const RepBlockW& blk = m.rep[sp.stage][sp.idx];
        const int step = (int)(&sp - c->m.steps.data());
        // range guard, site 1: the RepMixer's own output y is what the block's dw7x7 reads - max |y| into this step's slot
        const bool fused_half = blk.ffn.fused && c->use_fused_ffn && (c->batch_invariant || M >= kFusedFfnMinRows) && blk.ffn.precision == FVHD_FFN_HALF;
        unsigned* amax = (c->guard_active && c->guard_site == 1 && fused_half && step < c->guard_n) ? c->guard_dev + (size_t)step * kAmaxSlots : nullptr;
        // RepMixer dw3x3 and the ConvFFN's dw7x7 (+ BN) in ONE launch (round 6, csrc/dwconv_fused.hip: y crosses HBM once) wherever that kernel
        // takes the shape and the launch fills the chip; never in batch-invariant mode (its y may differ by one bf16 ulp from the VALU kernel's,
        // and the choice depends on the batch), never with the guard's maximum taken at site 1 (max |y|: that kernel only reduces max |A|)
        if (c->use_fused_dw && !c->batch_invariant && blk.mixer.K == 3 && blk.ffn.dw7.K == 7 && !(c->guard_active && c->guard_site == 1) &&
            fvhd_dw3_dw7_supported(B, H, H, C, 0)) {
            {
                Scope s(c, st, C_DWMIX);
                CHECK_LAUNCH(fvhd_launch_dw3_dw7(st, X, T, w.A, c->wp<float>(blk.mixer.w), c->wp<float>(blk.mixer.b), c->wp<float>(blk.ffn.dw7.w),
                                                 c->wp<float>(blk.ffn.dw7.b), B, H, H, C, ffn_amax_slot(c, blk.ffn, M, step)),
                             "dw3x3 -> dw7x7 launch");
            }
            std::swap(X, T);
            return run_ffn(c, st, blk.ffn, w, X, B, H, H, C, step, true);
        }
        if ((e = run_dw(c, st, C_DW3, blk.mixer, X, T, B, H, H, C, 1, 1, 0, amax))) return e;
        std::swap(X, T);
        return run_ffn(c, st, blk.ffn, w, X, B, H, H, C, step);
    }
    case S_ATT: {    // AttentionBlock (mci.py:1185-1188)
        const AttnBlockW& blk = m.att[sp.stage - 3][sp.idx];
        {
            Scope s(c, st, C_LN);
            CHECK_LAUNCH(fvhd_launch_layernorm(st, X, w.A, c->wp<float>(blk.ln_w), c->wp<float>(blk.ln_b), M, C, kLnEps),
                         "layernorm launch");
        }
        if ((e = run_gemm(c, st, C_QKV, c->wdev, blk.qkv, w.A, nullptr, nullptr, w.H, M, FVHD_EPI_NONE))) return e;
        {
            Scope s(c, st, C_ATT);
            CHECK_LAUNCH(fvhd_launch_attention(st, w.H, T, B, H * H, C, c->attn_fp8), "attention launch");
        }
        if ((e = run_gemm(c, st, C_PROJ, c->wdev, blk.proj, T, c->wp<float>(blk.ls1), X, X, M, FVHD_EPI_BIAS_LS_RESID, FVHD_BF16, w.part))) return e;
        return run_ffn(c, st, blk.ffn, w, X, B, H, H, C, (int)(&sp - c->m.steps.data()));
    }
    case S_DOWN: {   // PatchEmbed (mci.py:739-741)
        const DownW& d = m.down[sp.stage];
        if ((e = run_dw(c, st, C_DWDOWN, d.dw, X, T, B, H, H, C, 2, 2, 1))) return e;
        return run_gemm(c, st, C_1X1, c->wdev, d.pw, T, nullptr, nullptr, X, B * (H / 2) * (H / 2), FVHD_EPI_BIAS_GELU);
    }
    case S_HEAD: {   // conv_exp (mci.py:1401-1411, 1444) + feature_select (mobileclip_encoder.py:60-68)
        if ((e = run_dw(c, st, C_HEAD, m.conv_exp, X, T, B, H, H, C, 1, 2, 0))) return e;
        Scope s(c, st, C_HEAD);
        CHECK_LAUNCH(fvhd_launch_se_head(st, T, w.pooled, w.scale, c->wp<float>(m.se_wr), c->wp<float>(m.se_br),
                                         c->wp<float>(m.se_we), c->wp<float>(m.se_be), out, out_dtype, B, H * H, kOutDim, kSeRd),
                     "se head launch");
        return 0;
    }
    }
    return fail("run_step: bad step kind");
}

int prepare(fvhd_ctx* c, int B, hipStream_t st)          // the caller holds a DeviceGuard
{
    if (!c->finalized) return fail("fvhd: weights not finalized (call fvhd_finalize_weights)");
    if (B <= 0) return fail("fvhd: batch must be positive");
    return ensure_ws(c, B, st, true);
}

size_t dtype_size(int dt) { return dt == FVHD_F32 ? 4 : 2; }

// Steps [first, last] for the whole batch on `st` (X, T: the activation ping-pong buffers, updated in place).  The whole batch
// runs on the caller's stream: round 1-2 split it into two half-batches on two streams, which measured +0.4 % at B = 32 (the
// hardware does not co-schedule the MFMA-bound and the memory-bound kernels of the halves) and doubled the launch / graph logic.
int run_range(fvhd_ctx* c, hipStream_t st, int first, int last, const Ws& w, int B, char*& X, char*& T, const void* img,
              int img_dtype, void* out, int out_dtype)
{
    int e;
    for (int i = first; i <= last; ++i)
        if ((e = run_step(c, st, c->m.steps[i], w, X, T, B, img, img_dtype, out, out_dtype))) return e;
    return 0;
}

int encode_body(fvhd_ctx* c, const void* images, int img_dtype, int B, void* out, int out_dtype, hipStream_t st)
{
    int e;
    const Ws w = carve(c, c->ws, c->ws_batch, c->ws_hidden);
    const int n = (int)c->m.steps.size();
    char *X = w.X, *T = w.T;

    bool use_graph = c->graph && !c->prof && n >= 3;
    if (use_graph && is_capturing(st, true)) use_graph = false;     // a caller that is itself capturing gets plain launches (they land in its graph)
    if (!use_graph) return run_range(c, st, 0, n - 1, w, B, X, T, images, img_dtype, out, out_dtype);

    // ---- stem | graph of the interior steps | head ----
    if ((e = run_step(c, st, c->m.steps[0], w, X, T, B, images, img_dtype, nullptr, 0))) return e;
    const int fkey = (int)c->use_fused_ffn | (c->batch_invariant << 1) | (c->attn_fp8 << 2) | ((int)c->guard_active << 3) | (c->guard_site << 4);
    fvhd_ctx::GraphEntry* g = nullptr;
    for (auto& q : c->graphs)
        if (q.B == B && q.fused == fkey && q.ws == c->ws) g = &q;
    if (!g) {                              // first call with this key: eager (one-time kernel attributes are set on this pass)
        if ((e = run_range(c, st, 1, n - 2, w, B, X, T, nullptr, 0, nullptr, 0))) return e;
        c->graphs.push_back({B, fkey, c->ws, nullptr, false, X, T});
    } else if (g->failed) {
        if ((e = run_range(c, st, 1, n - 2, w, B, X, T, nullptr, 0, nullptr, 0))) return e;
    } else {
        if (!g->exec) {                    // second call: capture the same launch sequence instead of executing it
            hipGraph_t graph = nullptr;
            hipError_t he = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
            if (he == hipSuccess) {
                char *x = X, *t = T;
                e = run_range(c, st, 1, n - 2, w, B, x, t, nullptr, 0, nullptr, 0);
                he = hipStreamEndCapture(st, &graph);
                if (e == 0 && he == hipSuccess && graph) he = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
                else if (he == hipSuccess) he = hipErrorUnknown;
                if (graph) (void)hipGraphDestroy(graph);
            }
            if (he != hipSuccess || !g->exec) {       // leave the stream usable and fall back to plain launches for this key
                (void)hipGetLastError();
                g->exec = nullptr;
                g->failed = true;
                if ((e = run_range(c, st, 1, n - 2, w, B, X, T, nullptr, 0, nullptr, 0))) return e;
            }
        }
        if (g->exec) {
            hipError_t he = hipGraphLaunch(g->exec, st);
            if (he != hipSuccess) return hip_fail("hipGraphLaunch", he);
            X = g->X; T = g->T;
        }
    }
    return run_step(c, st, c->m.steps[n - 1], w, X, T, B, nullptr, 0, out, out_dtype);
}

int encode_impl(fvhd_ctx* c, const void* images, int img_dtype, int B, void* out, int out_dtype, hipStream_t st)
{
    if (img_dtype < 0 || img_dtype > 2 || out_dtype < 0 || out_dtype > 2) return fail("fvhd_encode: bad dtype");
    int e = prepare(c, B, st);
    if (e) return e;
    // ---- range guard: poll the earlier calls' read-backs, zero this call's slots; after the launches, read them back asynchronously.
    // Not while the caller captures the stream (an event recorded into a graph cannot be polled) - such callers calibrate up front.
    const bool capturing = is_capturing(st, true);
    if (capturing) c->ws_captured = true;                     // the caller's graph now holds pointers into this arena: retire it, never free it
    c->guard_active = c->guard_on && c->guard_dev && c->guard_n == (int)c->m.steps.size() && !capturing && !c->audit_dev;
    if (c->guard_active) {
        guard_process(c, false);
        const hipError_t he = hipMemsetAsync(c->guard_dev, 0, (size_t)c->guard_n * kAmaxSlots * 4, st);
        if (he != hipSuccess) { c->guard_active = false; return hip_fail("hipMemsetAsync(range guard)", he); }
    }
    e = encode_body(c, images, img_dtype, B, out, out_dtype, st);
    if (c->guard_active && !e) {
        GuardSlot& sl = c->guard_slots[c->guard_next];
        if (sl.pending) {                        // every slot in flight: the oldest one must finish first (a caller far ahead of the device)
            (void)hipEventSynchronize(sl.ev);
            sl.pending = false;
            if (guard_check_slot(c, sl)) { (void)hipDeviceSynchronize(); clear_graphs(c); }
        }
        hipError_t he = hipMemcpyAsync(sl.host, c->guard_dev, (size_t)c->guard_n * kAmaxSlots * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipEventRecord(sl.ev, st);
        if (he == hipSuccess) { sl.pending = true; c->guard_next = (c->guard_next + 1) % kGuardSlots; }
        else (void)hipGetLastError();            // the guard is best effort: a failed read-back never fails the encode
    }
    c->guard_active = false;
    return e;
}

int project_impl(fvhd_ctx* c, const void* tokens, int in_dtype, int rows, void* out, int out_dtype, hipStream_t st,
                 const Ws& w)
{
    const void* a = tokens;
    if (in_dtype != FVHD_BF16) {
        Scope s(c, st, C_PROJECTOR);
        CHECK_LAUNCH(fvhd_launch_cast_to_bf16(st, tokens, in_dtype, w.cast, (long)rows * c->mm_hidden), "cast launch");
        a = w.cast;
    }
    int e;
    if ((e = run_gemm(c, st, C_PROJECTOR, c->pdev, c->p0, a, nullptr, nullptr, w.ph, rows, FVHD_EPI_BIAS_GELU))) return e;
    return run_gemm(c, st, C_PROJECTOR, c->pdev, c->p2, w.ph, nullptr, nullptr, out, rows, FVHD_EPI_BIAS, out_dtype);
}

}  // namespace

// ===================================================================================================
extern "C" {

int fvhd_version(void) { return FVHD_VERSION; }

const char* fvhd_last_error(void) { return g_err.c_str(); }

// the other translation units of the library (the llm_*.hip C-ABI files) report through the same thread-local message; returns 1
int fvhd_set_error(const char* msg) { return fail(msg ? msg : "unknown error"); }

int fvhd_create(fvhd_ctx** out, int device, int image_size, int max_batch)
{
    if (!out) return fail("fvhd_create: out is NULL");
    *out = nullptr;
    if (image_size <= 0 || image_size % 64) return fail("fvhd_create: image_size must be a positive multiple of 64");
    if (max_batch <= 0) return fail("fvhd_create: max_batch must be positive");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail("fvhd_create: no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= n) return fail("fvhd_create: bad device index");
    DeviceGuard guard(device);               // (only validates the device here: nothing is allocated before fvhd_finalize_weights)
    if (guard.err != hipSuccess) return hip_fail("hipSetDevice", guard.err);
    fvhd_ctx* c = new fvhd_ctx();
    c->device = device;
    c->R = image_size;
    c->max_batch = max_batch;
    if (const char* ev = getenv("FVHD_FUSED_FFN")) c->use_fused_ffn = atoi(ev) != 0;
    if (const char* ev = getenv("FVHD_FUSED_DW")) c->use_fused_dw = atoi(ev) != 0;
    if (const char* ev = getenv("FVHD_GEMM_SPLITK")) c->use_splitk = atoi(ev) != 0;
    if (const char* ev = getenv("FVHD_FUSED_STEM")) c->use_fused_stem = atoi(ev);
    if (const char* ev = getenv("FVHD_ATTN_FP8")) c->attn_fp8 = atoi(ev) != 0;
    if (const char* ev = getenv("FVHD_GRAPH")) c->graph = atoi(ev) != 0;
    if (const char* ev = getenv("FVHD_RANGE_GUARD")) c->guard_on = atoi(ev) != 0;
    if (const char* ev = getenv("FVHD_GUARD_SITE")) c->guard_site = atoi(ev) != 0;
    *out = c;
    return 0;
}

void fvhd_destroy(fvhd_ctx* c)
{
    if (!c) return;
    DeviceGuard guard(c->device);
    (void)hipDeviceSynchronize();
    for (auto& r : c->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto& ev : c->ev_pool) (void)hipEventDestroy(ev);
    clear_graphs(c);
    guard_free(c);
    if (c->wdev) (void)hipFree(c->wdev);
    if (c->pdev) (void)hipFree(c->pdev);
    if (c->ws) (void)hipFree(c->ws);
    for (char* p : c->ws_retired) (void)hipFree(p);
    delete c;
}

int fvhd_set_tensor(fvhd_ctx* c, const char* key, const float* host_data, const int64_t* shape, int ndim)
{
    if (!c || !key || !host_data || ndim < 0 || ndim > 8) return fail("fvhd_set_tensor: bad argument");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(host_data, host_data + n);
    c->raw[key] = std::move(t);
    c->finalized = false;
    return 0;
}

int fvhd_finalize_weights(fvhd_ctx* c)
{
    if (!c) return fail("fvhd_finalize_weights: ctx is NULL");
    Packer pk;
    Model m;
    // ---- stem ----
    {
        const HostTensor* w = find(c, "patch_embed.0.reparam_conv.weight", {96, 3, 3, 3});
        const HostTensor* b = find(c, "patch_embed.0.reparam_conv.bias", {96});
        if (!w || !b) return 1;
        std::vector<float> t(27 * 96);
        for (int oc = 0; oc < 96; ++oc)
            for (int k = 0; k < 27; ++k) t[(size_t)k * 96 + oc] = w->data[(size_t)oc * 27 + k];   // k = ci*9 + ky*3 + kx
        m.stem0_w = pk.add_f32(t.data(), t.size());
        m.stem0_b = pk.add_f32(b->data.data(), 96);
    }
    if (!pack_dw(c, pk, "patch_embed.1.reparam_conv.weight", "patch_embed.1.reparam_conv.bias", 96, 3, &m.stem1)) return 1;
    if (!pack_gemm(c, pk, "patch_embed.2.reparam_conv.weight", "patch_embed.2.reparam_conv.bias", 96, 96, true, &m.stem2)) return 1;
    // ---- network entries in construction order (mci.py:1361-1399) ----
    int idx = 0;
    for (int s = 0; s < kStages; ++s) {
        const int C = kDims[s];
        if (s >= 3) {
            const std::string p = "network." + std::to_string(idx++);
            if (!pack_dw(c, pk, p + ".reparam_conv.weight", p + ".reparam_conv.bias", C, 7, &m.cpe[s - 3])) return 1;
        }
        const std::string ps = "network." + std::to_string(idx++);
        for (int b = 0; b < kLayers[s]; ++b) {
            const std::string p = ps + "." + std::to_string(b);
            if (s < 3) {
                RepBlockW blk;
                if (!pack_dw(c, pk, p + ".token_mixer.reparam_conv.weight", p + ".token_mixer.reparam_conv.bias", C, 3, &blk.mixer)) return 1;
                if (!pack_ffn(c, pk, p, p + ".layer_scale", C, &blk.ffn)) return 1;
                m.rep[s].push_back(blk);
            } else {
                AttnBlockW blk;
                if (!pack_vec(c, pk, p + ".norm.weight", {C}, &blk.ln_w)) return 1;
                if (!pack_vec(c, pk, p + ".norm.bias", {C}, &blk.ln_b)) return 1;
                if (!pack_vec(c, pk, p + ".layer_scale_1", {C, 1, 1}, &blk.ls1)) return 1;
                if (!pack_gemm(c, pk, p + ".token_mixer.qkv.weight", "", 3 * C, C, false, &blk.qkv)) return 1;
                if (!pack_gemm(c, pk, p + ".token_mixer.proj.weight", p + ".token_mixer.proj.bias", C, C, false, &blk.proj)) return 1;
                if (!pack_ffn(c, pk, p, p + ".layer_scale_2", C, &blk.ffn)) return 1;
                m.att[s - 3].push_back(blk);
            }
        }
        if (s < kStages - 1) {
            const std::string p = "network." + std::to_string(idx++);
            const int C2 = kDims[s + 1];
            if (!pack_dw(c, pk, p + ".proj.0.lkb_reparam.weight", p + ".proj.0.lkb_reparam.bias", C2, 7, &m.down[s].dw)) return 1;
            if (!pack_gemm(c, pk, p + ".proj.1.reparam_conv.weight", p + ".proj.1.reparam_conv.bias", C2, C2, true, &m.down[s].pw)) return 1;
        }
    }
    // ---- conv_exp + SE ----
    if (!pack_dw(c, pk, "conv_exp.reparam_conv.weight", "conv_exp.reparam_conv.bias", kOutDim, 3, &m.conv_exp)) return 1;
    if (!pack_vec(c, pk, "conv_exp.se.reduce.weight", {kSeRd, kOutDim, 1, 1}, &m.se_wr)) return 1;
    if (!pack_vec(c, pk, "conv_exp.se.reduce.bias", {kSeRd}, &m.se_br)) return 1;
    if (!pack_vec(c, pk, "conv_exp.se.expand.weight", {kOutDim, kSeRd, 1, 1}, &m.se_we)) return 1;
    if (!pack_vec(c, pk, "conv_exp.se.expand.bias", {kOutDim}, &m.se_be)) return 1;
    // head.proj (GlobalPool2D, mci.py:1290-1302) is dead on this path: feature_select drops the logits.
    // ---- step list ----
    m.steps.push_back(Step{S_STEM, 0, 0, 3, 1, kDims[0], 4});
    for (int s = 0, hd = 4; s < kStages; ++s, hd *= 2) {
        if (s >= 3) m.steps.push_back(Step{S_CPE, s, 0, kDims[s], hd, kDims[s], hd});
        for (int b = 0; b < kLayers[s]; ++b) m.steps.push_back(Step{s < 3 ? S_REP : S_ATT, s, b, kDims[s], hd, kDims[s], hd});
        if (s < kStages - 1) m.steps.push_back(Step{S_DOWN, s, 0, kDims[s], hd, kDims[s + 1], hd * 2});
        else m.steps.push_back(Step{S_HEAD, s, 0, kDims[s], hd, kOutDim, hd});
    }

    FVHD_ON_DEVICE(c);
    hipError_t e;
    (void)hipDeviceSynchronize();
    clear_graphs(c);                         // cached graphs point at the old packed weights
    if (c->wdev) (void)hipFree(c->wdev);
    c->wdev = nullptr;
    e = hipMalloc((void**)&c->wdev, pk.buf.size());
    if (e != hipSuccess) return hip_fail("hipMalloc(weights)", e);
    e = hipMemcpy(c->wdev, pk.buf.data(), pk.buf.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail("hipMemcpy(weights)", e);
    c->m = m;
    c->finalized = true;
    c->raw.clear();   // the packed image is the only copy the library keeps
    c->guard_hits.clear();
    if (int ge = guard_alloc(c, (int)c->m.steps.size())) return ge;
    return ensure_ws(c, c->max_batch);
}

int fvhd_set_projector(fvhd_ctx* c, const float* w0, const float* b0, const float* w2, const float* b2, int mm_hidden, int hidden)
{
    if (!c || !w0 || !b0 || !w2 || !b2) return fail("fvhd_set_projector: bad argument");
    if (mm_hidden % 32 || hidden % 32) return fail("fvhd_set_projector: mm_hidden and hidden must be multiples of 32");
    if (hidden <= 0 || mm_hidden <= 0) return fail("fvhd_set_projector: sizes must be positive");
    Packer pk;
    GemmW p0, p2;
    p0.w = pk.add_bf16(w0, (size_t)hidden * mm_hidden); p0.b = pk.add_f32(b0, hidden); p0.N = hidden; p0.K = mm_hidden; p0.has_bias = true;
    p2.w = pk.add_bf16(w2, (size_t)hidden * hidden); p2.b = pk.add_f32(b2, hidden); p2.N = hidden; p2.K = hidden; p2.has_bias = true;
    FVHD_ON_DEVICE(c);
    hipError_t e;
    (void)hipDeviceSynchronize();
    if (c->pdev) (void)hipFree(c->pdev);
    c->pdev = nullptr;
    e = hipMalloc((void**)&c->pdev, pk.buf.size());
    if (e != hipSuccess) return hip_fail("hipMalloc(projector)", e);
    e = hipMemcpy(c->pdev, pk.buf.data(), pk.buf.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail("hipMemcpy(projector)", e);
    c->p0 = p0; c->p2 = p2; c->mm_hidden = mm_hidden; c->hidden = hidden;
    return ensure_ws(c, c->ws_batch > 0 ? c->ws_batch : c->max_batch);
}

int fvhd_encode(fvhd_ctx* c, const void* images, int img_dtype, int batch, void* tokens_out, int out_dtype, fvhd_stream_t stream)
{
    if (!c || !images || !tokens_out) return fail("fvhd_encode: NULL argument");
    FVHD_ON_DEVICE(c);
    return encode_impl(c, images, img_dtype, batch, tokens_out, out_dtype, (hipStream_t)stream);
}

int fvhd_project(fvhd_ctx* c, const void* tokens, int in_dtype, int rows, void* out, int out_dtype, fvhd_stream_t stream)
{
    if (!c || !tokens || !out) return fail("fvhd_project: NULL argument");
    if (!c->pdev) return fail("fvhd_project: projector weights not set (call fvhd_set_projector)");
    if (rows <= 0) return fail("fvhd_project: rows must be positive");
    FVHD_ON_DEVICE(c);
    const int Tn = fvhd_num_tokens(c);
    int e = ensure_ws(c, (rows + Tn - 1) / Tn, (hipStream_t)stream, true);
    if (e) return e;
    if (is_capturing((hipStream_t)stream, true)) c->ws_captured = true;
    const Ws w = carve(c, c->ws, c->ws_batch, c->ws_hidden);
    return project_impl(c, tokens, in_dtype, rows, out, out_dtype, (hipStream_t)stream, w);
}

int fvhd_encode_images(fvhd_ctx* c, const void* images, int img_dtype, int batch, void* out, int out_dtype, fvhd_stream_t stream)
{
    if (!c || !images || !out) return fail("fvhd_encode_images: NULL argument");
    if (!c->pdev) return fail("fvhd_encode_images: projector weights not set (call fvhd_set_projector)");
    if (c->mm_hidden != kOutDim) return fail("fvhd_encode_images: the projector was set with mm_hidden != 3072 (the tower's token width)");
    if (batch <= 0) return fail("fvhd_encode_images: batch must be positive");
    FVHD_ON_DEVICE(c);
    int e = ensure_ws(c, batch, (hipStream_t)stream, true);
    if (e) return e;
    const Ws w = carve(c, c->ws, c->ws_batch, c->ws_hidden);
    e = encode_impl(c, images, img_dtype, batch, w.tok, FVHD_BF16, (hipStream_t)stream);
    if (e) return e;
    return project_impl(c, w.tok, FVHD_BF16, batch * fvhd_num_tokens(c), out, out_dtype, (hipStream_t)stream, w);
}

int fvhd_reserve(fvhd_ctx* c, int max_batch)
{
    if (!c) return fail("fvhd_reserve: ctx is NULL");
    if (max_batch <= 0) return fail("fvhd_reserve: max_batch must be positive");
    FVHD_ON_DEVICE(c);
    if (max_batch > c->max_batch) c->max_batch = max_batch;
    return c->finalized ? ensure_ws(c, max_batch) : 0;    // before fvhd_finalize_weights it only raises the size allocated there
}

int fvhd_num_steps(const fvhd_ctx* c) { return (c && c->finalized) ? (int)c->m.steps.size() : 0; }

int fvhd_step_info(const fvhd_ctx* c, int step, int* kind, int* stage, int* block, int* c_in, int* h_in, int* c_out, int* h_out)
{
    if (!c || !c->finalized) return fail("fvhd_step_info: weights not finalized");
    if (step < 0 || step >= (int)c->m.steps.size()) return fail("fvhd_step_info: bad step index");
    const Step& sp = c->m.steps[step];
    if (kind) *kind = sp.kind;
    if (stage) *stage = sp.stage;
    if (block) *block = sp.idx;
    if (c_in) *c_in = sp.C;
    if (h_in) *h_in = c->R / sp.hdiv;
    if (c_out) *c_out = sp.Cout;
    if (h_out) *h_out = c->R / sp.hdiv_out;
    return 0;
}

int fvhd_run_steps(fvhd_ctx* c, int first, int last, const void* x_in, int batch, void* x_out, fvhd_stream_t stream)
{
    if (!c || !x_in || !x_out) return fail("fvhd_run_steps: NULL argument");
    FVHD_ON_DEVICE(c);
    int e = prepare(c, batch, (hipStream_t)stream);
    if (e) return e;
    const int n = (int)c->m.steps.size();
    if (first < 0 || last >= n || first > last) return fail("fvhd_run_steps: bad step range");
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(c, c->ws, c->ws_batch, c->ws_hidden);
    char *X = w.X, *T = w.T;
    const Step& s0 = c->m.steps[first];
    const Step& s1 = c->m.steps[last];
    if (s0.kind != S_STEM) {
        const size_t hin = (size_t)(c->R / s0.hdiv);
        hipError_t he = hipMemcpyAsync(X, x_in, (size_t)batch * hin * hin * s0.C * 2, hipMemcpyDeviceToDevice, st);
        if (he != hipSuccess) return hip_fail("hipMemcpyAsync(x_in)", he);
    }
    for (int i = first; i <= last; ++i)
        if ((e = run_step(c, st, c->m.steps[i], w, X, T, batch, x_in, FVHD_BF16, x_out, FVHD_BF16))) return e;
    if (s1.kind != S_HEAD) {
        const size_t hout = (size_t)(c->R / s1.hdiv_out);
        hipError_t he = hipMemcpyAsync(x_out, X, (size_t)batch * hout * hout * s1.Cout * 2, hipMemcpyDeviceToDevice, st);
        if (he != hipSuccess) return hip_fail("hipMemcpyAsync(x_out)", he);
    }
    return 0;
}

int fvhd_num_tokens(const fvhd_ctx* c) { return c ? (c->R / 64) * (c->R / 64) : 0; }
int fvhd_hidden_size(const fvhd_ctx* c) { (void)c; return kOutDim; }

int fvhd_set_graph(fvhd_ctx* c, int on)
{
    if (!c) return fail("fvhd_set_graph: ctx is NULL");
    c->graph = on != 0;      // cached graphs stay valid (they are dropped when the workspace or the weights are replaced)
    return 0;
}

int fvhd_set_attention_fp8(fvhd_ctx* c, int on)
{
    if (!c) return fail("fvhd_set_attention_fp8: ctx is NULL");
    c->attn_fp8 = on != 0;       // (cached graphs are keyed by it)
    return 0;
}

int fvhd_set_batch_invariant(fvhd_ctx* c, int on)
{
    if (!c) return fail("fvhd_set_batch_invariant: ctx is NULL");
    c->batch_invariant = on != 0;
    return 0;
}

int fvhd_get_ffn_precision(const fvhd_ctx* c, int step)
{
    const FfnW* f = ffn_of_step(const_cast<fvhd_ctx*>(c), step);
    return (f && f->fused) ? f->precision : -1;      // -1: this step has no fused ConvFFN (its hidden tensor is bf16 in HBM: no f16 anywhere)
}

int fvhd_set_ffn_precision(fvhd_ctx* c, int step, int precision)
{
    FfnW* f = ffn_of_step(c, step);
    if (!f || !f->fused) return fail("fvhd_set_ffn_precision: step " + std::to_string(step) + " has no fused ConvFFN");
    if (precision != FVHD_FFN_HALF && precision != FVHD_FFN_BF16) return fail("fvhd_set_ffn_precision: precision must be FVHD_FFN_HALF or FVHD_FFN_BF16");
    if (f->precision != precision) {
        FVHD_ON_DEVICE(c);
        (void)hipDeviceSynchronize();
        clear_graphs(c);                     // cached graphs hold the other kernel and the other weight images
        f->precision = precision;
    }
    return 0;
}

int fvhd_set_range_guard(fvhd_ctx* c, int on)
{
    if (!c) return fail("fvhd_set_range_guard: ctx is NULL");
    c->guard_on = on != 0;       // (cached graphs are keyed by it)
    return 0;
}

int fvhd_range_guard_limit(const fvhd_ctx* c, int step, float* limit_out)
{
    const FfnW* f = ffn_of_step(const_cast<fvhd_ctx*>(c), step);
    if (!f || !f->fused || !limit_out) return fail("fvhd_range_guard_limit: step " + std::to_string(step) + " has no fused ConvFFN");
    *limit_out = c->guard_site == 1 ? f->guard_limit_y : f->guard_limit;      // the limit on the quantity the guard tracks (max |y| / max |A|)
    return 0;
}

int fvhd_range_guard_poll(fvhd_ctx* c, int wait, int* steps_out, float* amax_out, int max_out, int* n_out)
{
    if (!c || !n_out) return fail("fvhd_range_guard_poll: NULL argument");
    *n_out = 0;
    if (!c->finalized) return 0;
    FVHD_ON_DEVICE(c);
    guard_process(c, wait != 0);
    const int n = (int)c->guard_hits.size();
    for (int i = 0; i < n && i < max_out; ++i) {
        if (steps_out) steps_out[i] = c->guard_hits[i].step;
        if (amax_out) amax_out[i] = c->guard_hits[i].amax;
    }
    if (max_out <= 0) { *n_out = n; return 0; }     // count query: nothing is handed out, nothing is forgotten (round 6, advisor)
    *n_out = n < max_out ? n : max_out;
    if (n <= max_out) c->guard_hits.clear();
    else c->guard_hits.erase(c->guard_hits.begin(), c->guard_hits.begin() + max_out);
    return 0;
}

// Range audit of the fused ConvFFN's half-precision hidden activation (include/fvhd.h).  One eager pass over `images` with the fc1 output
// of every ConvFFN materialised and reduced to its max |.|; host-synchronising, never inside a stream capture.
int fvhd_audit_ranges(fvhd_ctx* c, const void* images, int img_dtype, int batch, float switch_above, float* max_abs_out, int* n_switched,
                      fvhd_stream_t stream)
{
    if (!c || !images) return fail("fvhd_audit_ranges: NULL argument");
    if (img_dtype < 0 || img_dtype > 2) return fail("fvhd_audit_ranges: bad dtype");
    FVHD_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    if (is_capturing(st)) return fail("fvhd_audit_ranges: not during stream capture (it reads its result back)");
    int e = prepare(c, batch, st);
    if (e) return e;
    const int n = (int)c->m.steps.size();
    unsigned* dev = nullptr;
    hipError_t he = hipMalloc((void**)&dev, (size_t)n * 4);
    if (he != hipSuccess) return hip_fail("hipMalloc(audit)", he);
    he = hipMemsetAsync(dev, 0, (size_t)n * 4, st);
    const Ws w = carve(c, c->ws, c->ws_batch, c->ws_hidden);
    char *X = w.X, *T = w.T;
    c->audit_dev = dev;
    if (he == hipSuccess) e = run_range(c, st, 0, n - 1, w, batch, X, T, images, img_dtype, w.tok, FVHD_BF16);   // tokens land in the workspace
    c->audit_dev = nullptr;
    std::vector<float> host((size_t)n, 0.f);
    if (he == hipSuccess && !e) he = hipMemcpyAsync(host.data(), dev, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && !e) he = hipStreamSynchronize(st);
    (void)hipFree(dev);
    if (e) return e;
    if (he != hipSuccess) return hip_fail("fvhd_audit_ranges", he);
    int switched = 0;
    for (int i = 0; i < n; ++i) {
        FfnW* f = ffn_of_step(c, i);
        // !(x <= limit) also catches NaN (an Inf / NaN in the fc1 output sorts above every finite value in the reduction)
        if (f && f->fused && switch_above > 0.f && !(host[i] <= switch_above) && f->precision != FVHD_FFN_BF16) {
            f->precision = FVHD_FFN_BF16;
            ++switched;
        }
    }
    if (switched) clear_graphs(c);
    if (max_abs_out) memcpy(max_abs_out, host.data(), (size_t)n * 4);
    if (n_switched) *n_switched = switched;
    return 0;
}

int fvhd_profile_enable(fvhd_ctx* c, int on)
{
    if (!c) return fail("fvhd_profile_enable: ctx is NULL");
    c->prof = on != 0;
    return 0;
}

static int drain(fvhd_ctx* c)
{
    for (auto& r : c->recs) {
        hipError_t e = hipEventSynchronize(r.b);
        if (e != hipSuccess) return hip_fail("hipEventSynchronize", e);
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, r.a, r.b);
        if (e != hipSuccess) return hip_fail("hipEventElapsedTime", e);
        c->acc_ms[r.cls] += ms;
        c->acc_n[r.cls] += 1;
        c->ev_pool.push_back(r.a);
        c->ev_pool.push_back(r.b);
    }
    c->recs.clear();
    return 0;
}

int fvhd_profile_reset(fvhd_ctx* c)
{
    if (!c) return fail("fvhd_profile_reset: ctx is NULL");
    FVHD_ON_DEVICE(c);
    int e = drain(c);
    for (int i = 0; i < C_COUNT; ++i) { c->acc_ms[i] = 0; c->acc_n[i] = 0; }
    return e;
}

int fvhd_profile_read(fvhd_ctx* c, int max_classes, const char** names, double* ms, int64_t* launches, int* n_classes)
{
    if (!c || !names || !ms || !launches || !n_classes) return fail("fvhd_profile_read: NULL argument");
    FVHD_ON_DEVICE(c);
    int e = drain(c);
    if (e) return e;
    int n = C_COUNT < max_classes ? C_COUNT : max_classes;
    for (int i = 0; i < n; ++i) { names[i] = kClassNames[i]; ms[i] = c->acc_ms[i]; launches[i] = c->acc_n[i]; }
    *n_classes = n;
    return 0;
}

// ---- single-op entry points -------------------------------------------------------------------------
int fvhd_op_dwconv(fvhd_stream_t st, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int Cin,
                   int K, int stride, int mult, int gelu)
{
    if (!x || !y || !w) return fail("fvhd_op_dwconv: NULL pointer");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || mult <= 0 || (Cin * mult) % 32)
        return fail("fvhd_op_dwconv: Cin * mult must be a positive multiple of 32 (got Cin=" + std::to_string(Cin) + " mult=" + std::to_string(mult) + ")");
    const bool known = (K == 3 && stride == 1 && mult == 1 && !gelu) || (K == 3 && stride == 2 && mult == 1 && gelu) ||
                       (K == 7 && stride == 1 && mult == 1 && !gelu) || (K == 7 && stride == 2 && mult == 2 && gelu) ||
                       (K == 3 && stride == 1 && mult == 2 && !gelu);
    if (!known) return fail("fvhd_op_dwconv: (K, stride, mult, gelu) must be one of (3,1,1,0) (3,2,1,1) (7,1,1,0) (7,2,2,1) (3,1,2,0)");
    int e = fvhd_launch_dwconv((hipStream_t)st, x, y, w, bias, B, H, W, Cin, K, stride, mult, gelu, 0, nullptr);
    return e ? hip_fail("fvhd_op_dwconv", (hipError_t)e) : 0;
}

// The ConvFFN's depthwise 7x7 (stride 1, folded BatchNorm bias) with the range guard's reduction: amax_bits (device, FVHD_AMAX_SLOTS = 64
// words, zeroed by the caller) receives max |y| as fp32 bit patterns of non-negative numbers - the maximum over the 64 words is the result.  mfma != 0: the matrix-core kernel (its shape rules), 0: the VALU kernel
int fvhd_op_dw7_amax(fvhd_stream_t st, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int C, int mfma, void* amax_bits)
{
    if (!x || !y || !w || !amax_bits) return fail("fvhd_op_dw7_amax: NULL pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 32) return fail("fvhd_op_dw7_amax: C must be a positive multiple of 32");
    int e;
    if (mfma) {
        if (!fvhd_dw7_mfma_supported(B, H, W, C, 1)) return fail("fvhd_op_dw7_amax: shape not supported by the matrix-core kernel");
        e = fvhd_launch_dw7_mfma((hipStream_t)st, x, y, w, bias, B, H, W, C, (unsigned*)amax_bits);
    } else {
        // the dispatcher of fvhd_launch_dwconv hands a shape to the matrix-core kernel exactly when fvhd_dw7_mfma_supported(..., 0) holds: refuse
        // those here, so that "mfma = 0" always means the VALU kernel ran
        if (fvhd_dw7_mfma_supported(B, H, W, C, 0)) return fail("fvhd_op_dw7_amax: this shape dispatches to the matrix-core kernel (pass mfma = 1)");
        e = fvhd_launch_dwconv((hipStream_t)st, x, y, w, bias, B, H, W, C, 7, 1, 1, 0, 0, (unsigned*)amax_bits);
    }
    return e ? hip_fail("fvhd_op_dw7_amax", (hipError_t)e) : 0;
}

int fvhd_op_gemm(fvhd_stream_t st, const void* A, const void* Wt, const float* bias, const float* ls, const void* resid,
                 void* out, int M, int N, int K, int epilogue, int out_dtype)
{
    if (!A || !Wt || !out) return fail("fvhd_op_gemm: NULL pointer");
    if ((epilogue == FVHD_EPI_BIAS || epilogue == FVHD_EPI_BIAS_GELU || epilogue == FVHD_EPI_BIAS_LS_RESID) && !bias) return fail("fvhd_op_gemm: this epilogue needs bias");
    if (epilogue == FVHD_EPI_BIAS_LS_RESID && !ls) return fail("fvhd_op_gemm: FVHD_EPI_BIAS_LS_RESID needs ls");
    if ((epilogue == FVHD_EPI_BIAS_LS_RESID || epilogue == FVHD_EPI_RESID) && !resid) return fail("fvhd_op_gemm: this epilogue needs resid");
    int e = fvhd_launch_gemm((hipStream_t)st, A, Wt, bias, ls, resid, out, M, N, K, epilogue, out_dtype);
    return e ? hip_fail("fvhd_op_gemm", (hipError_t)e) : 0;
}

int fvhd_op_gemm_splitk_ls(fvhd_stream_t st, const void* A, const void* Wt, const float* bias, const float* ls, const void* resid, void* out,
                           float* partial, int M, int N, int K, int splits)
{
    if (!A || !Wt || !bias || !ls || !resid || !out || !partial) return fail("fvhd_op_gemm_splitk_ls: NULL pointer");
    int e = fvhd_launch_gemm_splitk_ls((hipStream_t)st, A, Wt, bias, ls, resid, out, partial, M, N, K, splits);
    return e ? hip_fail("fvhd_op_gemm_splitk_ls", (hipError_t)e) : 0;
}

int fvhd_op_layernorm(fvhd_stream_t st, const void* x, void* y, const float* w, const float* b, int M, int C, float eps)
{
    int e = fvhd_launch_layernorm((hipStream_t)st, x, y, w, b, M, C, eps);
    return e ? hip_fail("fvhd_op_layernorm", (hipError_t)e) : 0;
}

int fvhd_op_attention(fvhd_stream_t st, const void* qkv, void* out, int B, int N, int C)
{
    int e = fvhd_launch_attention((hipStream_t)st, qkv, out, B, N, C, 0);
    return e ? hip_fail("fvhd_op_attention", (hipError_t)e) : 0;
}

int fvhd_op_attention_fp8(fvhd_stream_t st, const void* qkv, void* out, int B, int N, int C)
{
    int e = fvhd_launch_attention((hipStream_t)st, qkv, out, B, N, C, 1);
    return e ? hip_fail("fvhd_op_attention_fp8", (hipError_t)e) : 0;
}

int fvhd_op_stem_conv(fvhd_stream_t st, const void* img, int dtype, void* out, const float* w, const float* bias, int B, int R)
{
    int e = fvhd_launch_stem_conv((hipStream_t)st, img, dtype, out, w, bias, B, R);
    return e ? hip_fail("fvhd_op_stem_conv", (hipError_t)e) : 0;
}

int fvhd_op_stem_fused(fvhd_stream_t st, const void* img, int dtype, void* out, const float* w0, const float* b0,
                       const float* w1, const float* b1, const void* w2, const float* b2, int B, int R)
{
    if ((w2 == nullptr) != (b2 == nullptr)) return fail("fvhd_op_stem_fused: w2 and b2 come together");
    int e = fvhd_launch_stem_fused((hipStream_t)st, img, dtype, out, w0, b0, w1, b1, w2, b2, B, R);
    return e ? hip_fail("fvhd_op_stem_fused", (hipError_t)e) : 0;
}

int fvhd_op_se_head(fvhd_stream_t st, const void* y, float* pooled, float* scale, const float* wr, const float* br,
                    const float* we, const float* be, void* out, int out_dtype, int B, int T, int C, int RD)
{
    int e = fvhd_launch_se_head((hipStream_t)st, y, pooled, scale, wr, br, we, be, out, out_dtype, B, T, C, RD);
    return e ? hip_fail("fvhd_op_se_head", (hipError_t)e) : 0;
}

int fvhd_op_dw3_dw7(fvhd_stream_t st, const void* x, void* y, void* a, const float* w3, const float* b3, const float* w7, const float* b7,
                    int B, int H, int W, int C, void* amax_bits)
{
    if (!x || !y || !a || !w3 || !w7) return fail("fvhd_op_dw3_dw7: NULL pointer");
    if (x == y || x == a || y == a) return fail("fvhd_op_dw3_dw7: x, y and a must be three distinct buffers");
    if (!fvhd_dw3_dw7_supported(B, H, W, C, 1))
        return fail("fvhd_op_dw3_dw7: needs C % 32 == 0, C >= 64, W % 4 == 0, W >= 16 and an image below 2 GiB (got B=" + std::to_string(B) + " H=" +
                    std::to_string(H) + " W=" + std::to_string(W) + " C=" + std::to_string(C) + ")");
    int e = fvhd_launch_dw3_dw7((hipStream_t)st, x, y, a, w3, b3, w7, b7, B, H, W, C, (unsigned*)amax_bits);
    return e ? hip_fail("fvhd_op_dw3_dw7", (hipError_t)e) : 0;
}

// PatchEmbed's dw7x7 / stride 2 / multiplier 2 + bias + GELU on the matrix-core kernel directly (also for maps the dispatcher leaves to the VALU kernel)
int fvhd_op_dw7s2_mfma(fvhd_stream_t st, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int Cin)
{
    if (!x || !y || !w) return fail("fvhd_op_dw7s2_mfma: NULL pointer");
    if (!fvhd_dw7s2_mfma_supported(B, H, W, Cin, 1))
        return fail("fvhd_op_dw7s2_mfma: needs Cin % 32 == 0, H, W >= 2 and images below 2 GiB (got B=" + std::to_string(B) + " H=" +
                    std::to_string(H) + " W=" + std::to_string(W) + " Cin=" + std::to_string(Cin) + ")");
    int e = fvhd_launch_dw7s2_mfma((hipStream_t)st, x, y, w, bias, B, H, W, Cin, 1);
    return e ? hip_fail("fvhd_op_dw7s2_mfma", (hipError_t)e) : 0;
}

int fvhd_op_dw7_mfma(fvhd_stream_t st, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int C)
{
    if (!x || !y || !w) return fail("fvhd_op_dw7_mfma: NULL pointer");
    if (!fvhd_dw7_mfma_supported(B, H, W, C, 1))
        return fail("fvhd_op_dw7_mfma: needs C % 64 == 0 or C % 96 == 0, W >= 16 and an image below 2 GiB (got B=" + std::to_string(B) + " H=" +
                    std::to_string(H) + " W=" + std::to_string(W) + " C=" + std::to_string(C) + ")");
    int e = fvhd_launch_dw7_mfma((hipStream_t)st, x, y, w, bias, B, H, W, C, nullptr);
    return e ? hip_fail("fvhd_op_dw7_mfma", (hipError_t)e) : 0;
}

int fvhd_op_preprocess(fvhd_stream_t st, const void* src, int src_h, int src_w, int64_t src_pitch, int pad_top, int pad_left, uint32_t bg,
                       const int32_t* hbounds, const int32_t* hcoef, int hk, const int32_t* vbounds, const int32_t* vcoef, int vk, int row0,
                       int nrows, void* tmp, const float* lut, int R, void* out, int out_dtype)
{
    if (!src || !hbounds || !hcoef || !vbounds || !vcoef || !tmp || !lut || !out) return fail("fvhd_op_preprocess: NULL pointer");
    if (src_pitch < 3ll * src_w) return fail("fvhd_op_preprocess: src_pitch smaller than a row of RGB pixels");
    int e = fvhd_launch_preprocess((hipStream_t)st, src, src_h, src_w, (long)src_pitch, pad_top, pad_left, bg, hbounds, hcoef, hk, vbounds, vcoef,
                                   vk, row0, nrows, tmp, lut, R, out, out_dtype);
    return e ? hip_fail("fvhd_op_preprocess", (hipError_t)e) : 0;
}

int fvhd_op_ffn_fused(fvhd_stream_t st, const void* A, const void* w1img, const float* b1, const void* w2img, const float* b2,
                      const float* ls, void* X, int M, int C, int precision)
{
    if (precision != FVHD_FFN_HALF && precision != FVHD_FFN_BF16) return fail("fvhd_op_ffn_fused: precision must be FVHD_FFN_HALF or FVHD_FFN_BF16");
    int e = fvhd_launch_ffn_fused((hipStream_t)st, A, w1img, b1, w2img, b2, ls, X, M, C, precision);
    return e ? hip_fail("fvhd_op_ffn_fused", (hipError_t)e) : 0;
}

int fvhd_op_splice(fvhd_stream_t st, const int64_t* ids, const int32_t* start, const int32_t* seqlen, const int64_t* feat_row0,
                   const int64_t* labels_in, const void* table, const void* feats, void* out, uint8_t* mask_out, int64_t* pos_out,
                   int64_t* labels_out, int B, int L, int H, int max_len, int64_t vocab, int64_t n_feat_rows, int left_pad, int dtype)
{
    if (!ids || !start || !seqlen || !feat_row0 || !table || !feats || !out) return fail("fvhd_op_splice: NULL argument");
    if (dtype < 0 || dtype > 2) return fail("fvhd_op_splice: bad dtype");
    int e = fvhd_launch_splice((hipStream_t)st, (const long*)ids, start, seqlen, (const long*)feat_row0, (const long*)labels_in, table, feats,
                               out, mask_out, (long*)pos_out, (long*)labels_out, B, L, H, max_len, (long)vocab, (long)n_feat_rows, left_pad, dtype);
    return e ? hip_fail("fvhd_op_splice", (hipError_t)e) : 0;
}

int fvhd_ffn_pack(int C, const float* host_fc1, const float* host_fc2, void* host_w1img, void* host_w2img, int precision)
{
    if (!host_fc1 || !host_fc2 || !host_w1img || !host_w2img) return fail("fvhd_ffn_pack: NULL argument");
    if (fvhd_ffn_pack_host(C, host_fc1, host_fc2, (uint16_t*)host_w1img, (uint16_t*)host_w2img, precision))
        return fail("fvhd_ffn_pack: the fused ConvFFN kernel exists for C in {96, 192, 384}, precision FVHD_FFN_HALF / FVHD_FFN_BF16");
    return 0;
}

}  // extern "C"
