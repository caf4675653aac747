// C ABI of the Qwen2 prefill (include/fvhd.h "LLM prefill"): context, weight packing, workspace and the launch sequence of
// transformers' Qwen2ForCausalLM.forward on inputs_embeds (the call the reference makes at llava/model/language_model/
// llava_qwen.py:92-103 after prepare_inputs_labels_for_multimodal, and from generate(), :138-143).  Kernels: llm.hip + gemm.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/fvhd.h"
#include "llm_decode.h"

extern "C" {
int fvhd_launch_gemm(hipStream_t, const void*, const void*, const float*, const float*, const void*, void*, int, int, int, int, int);
int fvhd_launch_gemm_splitk(hipStream_t, const void*, const void*, const void*, void*, float*, int, int, int, int);
int fvhd_launch_gemm_splitk_partials(hipStream_t, const void*, const void*, float*, int, int, int, int);
int fvhd_launch_splitk_bias_rope(hipStream_t, const float*, int, int, const float*, void*, const long*, const float*, void*, void*, int, int, int, int, int, int, float);
int fvhd_launch_gemm_splitk_norm(hipStream_t, const void*, const void*, const void*, void*, float*, int, int, int, int, const float*, void*, float);
int fvhd_launch_rmsnorm(hipStream_t, const void*, void*, const float*, int, int, float);
int fvhd_launch_rope(hipStream_t, void*, const long*, const float*, void*, void*, int, int, int, int, int, int, float);
int fvhd_gemm_qkv_rope_supported(int, int, int, int, int, int);
int fvhd_launch_gemm_qkv_rope(hipStream_t, const void*, const void*, const float*, void*, int, int, int, const long*, const float*, void*, void*, int, int, int, int, int, int, float);
int fvhd_launch_llm_attention(hipStream_t, const void*, void*, const unsigned char*, int, int, int, int, int);
int fvhd_launch_cast_rows(hipStream_t, const void*, int, void*, long);
int fvhd_launch_gather_rows(hipStream_t, const void*, void*, int, int, int, int);
int fvhd_set_error(const char* msg);     // fvhd_api.hip: the library's one thread-local error string
// llm_decode.hip
int fvhd_launch_dec_gemm(hipStream_t, const DecGemmArgs*);
int fvhd_launch_dec_attention(hipStream_t, const void*, const void*, const void*, const unsigned char*, void*, int, int, int, int, int, const int*, int, int, int,
                              float*, int*, const int*);
int fvhd_launch_dec_embed(hipStream_t, const int64_t*, const int64_t*, const void*, int, int, void*, unsigned char*, int, int, const int*, int*, int*);
int fvhd_launch_dec_argmax_finish(hipStream_t, const float*, const int*, int, int, int64_t*, int64_t*, int64_t*, int*, const int*);
int fvhd_launch_dec_argmax_blocks(hipStream_t, const float*, int, int, float*, int*);
int fvhd_launch_dec_start_state(hipStream_t, int64_t*, const int64_t*, int, int, int*, int*);
// llm_w8.hip
int fvhd_launch_quantize_e4m3(hipStream_t, const void*, int, int, void*, long, float*, int, int);
int fvhd_launch_w8_unpack(hipStream_t, const void*, const float*, void*, long, int, int);
int fvhd_launch_dec_embed_w8(hipStream_t, const int64_t*, const int64_t*, const void*, const float*, int, int, void*, unsigned char*, int, int, const int*, int*, int*);
// llm_sample.hip
size_t fvhd_dec_sample_ws_bytes(void);
int fvhd_launch_dec_sample(hipStream_t, const DecSampleArgs*, void*);
}

namespace {

constexpr int EPI_NONE = 0, EPI_BIAS = 1, EPI_RESID = 4, EPI_SWIGLU = 5;
constexpr int kMaxSplits = 4;

int lfail(const std::string& m) { return fvhd_set_error(m.c_str()); }
int lhip(const char* what, hipError_t e) { return lfail(std::string(what) + ": " + hipGetErrorString(e)); }

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

uint16_t bf16_rne(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

float half_to_float(uint16_t h)
{
    const uint32_t s = (uint32_t)(h & 0x8000) << 16, e = (h >> 10) & 31, m = h & 1023;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = s;
        else { int k = 0; uint32_t mm = m; while (!(mm & 1024)) { mm <<= 1; ++k; } u = s | ((uint32_t)(113 - k) << 23) | ((mm & 1023) << 13); }
    } else if (e == 31) u = s | 0x7f800000u | (m << 13);
    else u = s | ((e + 112) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

float load_as_float(const void* p, int dtype, size_t i)
{
    if (dtype == FVHD_F32) return ((const float*)p)[i];
    if (dtype == FVHD_BF16) { uint32_t u = (uint32_t)((const uint16_t*)p)[i] << 16; float f; memcpy(&f, &u, 4); return f; }
    return half_to_float(((const uint16_t*)p)[i]);
}

struct LayerOff { size_t ln1, wqkv, bqkv, wo, ln2, wgu, wd, sqkv, so, sgu, sd; };     // s*: the fp32 row scales of an e4m3 matrix

struct DevGuard {
    int prev = -1; bool sw = false; hipError_t err = hipSuccess;
    explicit DevGuard(int d) { err = hipGetDevice(&prev); if (err == hipSuccess && prev != d) { err = hipSetDevice(d); sw = err == hipSuccess; } }
    ~DevGuard() { if (sw) (void)hipSetDevice(prev); }
};

}  // namespace

struct fvhd_llm {
    int device = 0, H = 0, L = 0, nh = 0, nkv = 0, hd = 0, I = 0, V = 0;
    float eps = 1e-6f, theta = 1e6f;
    int qkvw = 0;
    char* wdev = nullptr;
    size_t wbytes = 0;
    std::vector<LayerOff> lo;
    size_t norm_off = 0, lm_off = 0, lm_soff = 0;
    int wfmt = FVHD_W_BF16;                // fvhd_llm_set_weight_format: FVHD_W_E4M3 = every matrix as e4m3 codes (1 byte, the K order of llm_w8.hip) + one
                                           // fp32 scale per row; vectors and model.embed_tokens.weight are not affected
    bool any_set = false;                  // a tensor was set: the format is fixed
    char* wscratch = nullptr;              // e4m3: bf16 scratch of the largest matrix - the prefill dequantises each matrix into it right before its GEMM
    size_t wscratch_bytes = 0;
    std::vector<char> got;                 // per expected tensor: received?
    std::vector<std::string> names;
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    int ws_rows = 0, ws_batch = 0, ws_pos = 0;
    char *h = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *act = nullptr, *last = nullptr, *lastn = nullptr;
    float *rope = nullptr, *part = nullptr;
    int fuse_rope = 0;                     // FVHD_LLM_FUSEROPE=1: rotary embedding + KV-cache copies inside the q|k|v projection's epilogue instead of their own launch (identical bits; measured neutral - prefill 3.421 / 3.410 -> 3.404 / 3.407 ms at B = 8, 2.316 -> 2.342 at B = 1, profiles/r05_ttft_fuserope_ab.log: the 5.4-us launch saved comes back as epilogue time - so off by default)
    int down_splits = kMaxSplits, o_splits = 2, qkv_splits = 0, fuse_norm = 1;     // FVHD_LLM_SPLITK / FVHD_LLM_OSPLIT (largest split of down_proj / o_proj, 0 = never) / FVHD_LLM_QKVSPLIT / FVHD_LLM_FUSENORM
    int max_pos = 0;                       // fvhd_llm_set_max_positions (config.max_position_embeddings): rows of the rotary table
    // A prefill that ran while its stream was being captured put this workspace's pointers into the CALLER's graph.  Such a workspace is
    // never freed when a later call needs a bigger one: it is retired (kept until fvhd_llm_destroy), so the captured graph keeps
    // replaying on valid memory.  `generation` counts workspace replacements (fvhd_llm_workspace_generation).
    bool ws_captured = false;
    std::vector<char*> retired;
    int generation = 0;
    // fvhd_llm_set_tensor_device enqueues its copies on the CALLER's stream: `load_ev` is recorded behind the latest one so that
    // fvhd_llm_finalize (host wait) and fvhd_llm_prefill (stream wait, whatever stream it runs on) are ordered after the packing
    hipEvent_t load_ev = nullptr;
    hipStream_t load_stream = nullptr;
    bool load_pending = false;
    // ---- decode (fvhd_llm_cache_reserve / start / decode) ----
    char* emb = nullptr;                   // model.embed_tokens.weight, bf16 [V][H]: optional, the decode's input table of an untied model
    int tied = -1;                         // fvhd_llm_set_tied_embeddings: 1 = the decode embeds through the packed lm_head rows, 0 = through
                                           // `emb`; -1 = not said - the decode then needs `emb` (it never guesses the lm_head rows)
    char* dc = nullptr;                    // one allocation: caches, mask, device words, decode workspace, rotary table
    size_t dc_bytes = 0;
    int dc_batch = 0, dc_cap = 0, dc_pos = 0;
    int run_batch = 0;                     // batch of the last fvhd_llm_start (the decode steps run on it)
    char *kcache = nullptr, *vcache = nullptr, *dh = nullptr, *dq = nullptr, *datt = nullptr, *dact = nullptr;
    unsigned char* mask = nullptr;
    int64_t *posv = nullptr, *last_ids = nullptr;
    int *len = nullptr, *status = nullptr, *cnt = nullptr, *amax_i = nullptr;
    float *dpart = nullptr, *apart = nullptr, *amax_v = nullptr, *dlogits = nullptr, *drope = nullptr, *drstd = nullptr;
    int dec_rstd_once = 1;                 // a decode GEMM with a folded norm above 16 rows: the row statistics from one small launch (dec_rstd_kernel)
                                           // instead of every workgroup; FVHD_DEC_RSTD_ONCE=0 for the A/B (identical bits)
    int* status_host = nullptr;            // host-mapped copy of the error word: read by every host call without a synchronisation
    int* status_host_dev = nullptr;
    int cnt_att = 0;                       // counters [0, cnt_att) of the GEMMs, then B * nh of the attention
    struct Plan { int S = 1, cpw = 1; } p_qkv, p_o, p_gu, p_d, p_lm;
    int att_S = 1, att_chunk = 0;
    char* pre_kv = nullptr;                // the prefill's own [n_layers][batch][nkv][seq_len][hd] caches, copied into the strided ones
    size_t pre_kv_bytes = 0;
    // fvhd_llm_set_sampling: read when fvhd_llm_start / fvhd_llm_decode enqueue (a captured graph keeps what it was captured with)
    int do_sample = 0;
    float temperature = 1.f, top_p = 1.f;
    int top_k = 0;
    unsigned long long seed = 0;
    char* sws = nullptr;                   // the sampler's workspace (inside `dc`)
};

namespace {

// expected tensor index: per layer 12 (ln1, q.w, q.b, k.w, k.b, v.w, v.b, o.w, ln2, gate, up, down), then norm, lm_head
int tensor_index(const fvhd_llm* c, const std::string& key, int* layer, int* which)
{
    std::string k = key;
    if (k.rfind("model.", 0) == 0) k = k.substr(6);
    if (k == "norm.weight") { *layer = -1; *which = 0; return c->L * 12; }
    if (k == "lm_head.weight") { *layer = -1; *which = 1; return c->L * 12 + 1; }
    if (k.rfind("layers.", 0) != 0) return -1;
    const size_t dot = k.find('.', 7);
    if (dot == std::string::npos) return -1;
    const int l = atoi(k.substr(7, dot - 7).c_str());
    if (l < 0 || l >= c->L) return -1;
    const std::string rest = k.substr(dot + 1);
    static const char* kNames[12] = {"input_layernorm.weight", "self_attn.q_proj.weight", "self_attn.q_proj.bias", "self_attn.k_proj.weight",
                                     "self_attn.k_proj.bias", "self_attn.v_proj.weight", "self_attn.v_proj.bias", "self_attn.o_proj.weight",
                                     "post_attention_layernorm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight"};
    for (int i = 0; i < 12; ++i)
        if (rest == kNames[i]) { *layer = l; *which = i; return l * 12 + i; }
    return -1;
}

bool is_embed_key(const char* key)
{
    const std::string k(key);
    return k == "model.embed_tokens.weight" || k == "embed_tokens.weight";
}

// offsets of the packed weights in `wdev` for the context's weight format -> c->lo, norm_off, lm_off, lm_soff, wbytes
void weight_layout(fvhd_llm* c)
{
    const size_t H = c->H, I = c->I, qkvw = c->qkvw, ao = (size_t)c->nh * c->hd, V = c->V;
    const bool q8 = c->wfmt == FVHD_W_E4M3;
    const size_t eb = q8 ? 1 : 2;          // bytes per matrix element
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al256(bytes); return o; };
    c->lo.assign(c->L, LayerOff{});
    for (int l = 0; l < c->L; ++l) {
        LayerOff& o = c->lo[l];
        o.ln1 = take(H * 4);
        o.wqkv = take(qkvw * H * eb);
        o.bqkv = take(qkvw * 4);
        o.wo = take(H * ao * eb);
        o.ln2 = take(H * 4);
        o.wgu = take(2 * I * H * eb);
        o.wd = take(H * I * eb);
        if (q8) { o.sqkv = take(qkvw * 4); o.so = take(H * 4); o.sgu = take(2 * I * 4); o.sd = take(H * 4); }
    }
    c->norm_off = take(H * 4);
    c->lm_off = take(V * H * eb);
    c->lm_soff = q8 ? take(V * 4) : 0;
    c->wbytes = off;
}

// where a tensor of the state dict goes: cols == 0: `rows` floats at base + 4 eoff; else a [rows][cols] matrix whose element (0, 0) is
// element eoff of the packed matrix at `base`, rows `pitch` elements apart (gate / up: interleaved rows), and - e4m3 - whose row scales
// start at float seoff of `sbase`, one every `sstride` floats
struct Slot { size_t base = 0, eoff = 0, rows = 0, cols = 0, pitch = 0, sbase = 0, seoff = 0; int sstride = 1; };

Slot slot_of(const fvhd_llm* c, int layer, int which)
{
    const size_t H = c->H, hd = c->hd, nh = c->nh, nkv = c->nkv, I = c->I;
    Slot s;
    if (layer < 0) {
        if (which == 0) { s.base = c->norm_off; s.rows = H; }
        else { s.base = c->lm_off; s.rows = c->V; s.cols = H; s.pitch = H; s.sbase = c->lm_soff; }
        return s;
    }
    const LayerOff& o = c->lo[layer];
    switch (which) {
    case 0: s.base = o.ln1; s.rows = H; break;
    case 1: s.base = o.wqkv; s.rows = nh * hd; s.cols = H; s.pitch = H; s.sbase = o.sqkv; break;
    case 2: s.base = o.bqkv; s.rows = nh * hd; break;
    case 3: s.base = o.wqkv; s.eoff = nh * hd * H; s.rows = nkv * hd; s.cols = H; s.pitch = H; s.sbase = o.sqkv; s.seoff = nh * hd; break;
    case 4: s.base = o.bqkv; s.eoff = nh * hd; s.rows = nkv * hd; break;
    case 5: s.base = o.wqkv; s.eoff = (nh + nkv) * hd * H; s.rows = nkv * hd; s.cols = H; s.pitch = H; s.sbase = o.sqkv; s.seoff = (nh + nkv) * hd; break;
    case 6: s.base = o.bqkv; s.eoff = (nh + nkv) * hd; s.rows = nkv * hd; break;
    case 7: s.base = o.wo; s.rows = H; s.cols = nh * hd; s.pitch = nh * hd; s.sbase = o.so; break;
    case 8: s.base = o.ln2; s.rows = H; break;
    // gate / up rows interleaved (row 2j = gate_j, row 2j + 1 = up_j): the SwiGLU epilogue of the GEMM pairs adjacent columns
    case 9: s.base = o.wgu; s.rows = I; s.cols = H; s.pitch = 2 * H; s.sbase = o.sgu; s.sstride = 2; break;
    case 10: s.base = o.wgu; s.eoff = H; s.rows = I; s.cols = H; s.pitch = 2 * H; s.sbase = o.sgu; s.seoff = 1; s.sstride = 2; break;
    case 11: s.base = o.wd; s.rows = H; s.cols = I; s.pitch = I; s.sbase = o.sd; break;
    }
    return s;
}

// e4m3: bf16 rows [rows][cols] on the device -> codes + scales at the slot (rows are whole, so every source tensor quantises on its own)
int quantize_into(fvhd_llm* c, const Slot& s, const void* dev_bf16, hipStream_t st)
{
    const int e = fvhd_launch_quantize_e4m3(st, dev_bf16, (int)s.rows, (int)s.cols, c->wdev + s.base + s.eoff, (long)s.pitch,
                                            (float*)(c->wdev + s.sbase) + s.seoff, s.sstride, 1);
    return e ? lhip("quantise to e4m3", (hipError_t)e) : 0;
}

int ensure_emb(fvhd_llm* c)
{
    if (c->emb) return 0;
    const hipError_t e = hipMalloc((void**)&c->emb, (size_t)c->V * c->H * 2);
    return e == hipSuccess ? 0 : lhip("hipMalloc(embed_tokens)", e);
}

// host rows [rows][cols] of `dtype` -> device bf16 rows at dst, dst row pitch `pitch_elems` (interleaving = pitch 2 * cols)
int upload_matrix(const void* host, int dtype, size_t rows, size_t cols, char* dst, size_t pitch_elems)
{
    std::vector<uint16_t> tmp(rows * cols);
    if (dtype == FVHD_BF16) memcpy(tmp.data(), host, rows * cols * 2);
    else
        for (size_t i = 0; i < rows * cols; ++i) tmp[i] = bf16_rne(load_as_float(host, dtype, i));
    hipError_t e = hipMemcpy2D(dst, pitch_elems * 2, tmp.data(), cols * 2, cols * 2, rows, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : lhip("hipMemcpy2D(llm weights)", e);
}

// e4m3: the same host rows through a bf16 staging buffer on the device and the quantise kernel
int upload_matrix_q(fvhd_llm* c, const void* host, int dtype, const Slot& s)
{
    char* stage = nullptr;
    hipError_t e = hipMalloc((void**)&stage, s.rows * s.cols * 2);
    if (e != hipSuccess) return lhip("hipMalloc(quantise staging)", e);
    int r = upload_matrix(host, dtype, s.rows, s.cols, stage, s.cols);
    if (!r) r = quantize_into(c, s, stage, nullptr);
    if (!r && (e = hipStreamSynchronize(nullptr)) != hipSuccess) r = lhip("hipStreamSynchronize(quantise)", e);
    (void)hipFree(stage);
    return r;
}

int upload_vector_f32(const void* host, int dtype, size_t n, char* dst)
{
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = load_as_float(host, dtype, i);
    hipError_t e = hipMemcpy(dst, tmp.data(), n * 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : lhip("hipMemcpy(llm vector)", e);
}

int ensure_ws(fvhd_llm* c, int B, int T, hipStream_t st, bool check_capture)
{
    const int rows = (int)(((size_t)B * T + 255) / 256 * 256);
    if (c->ws && rows <= c->ws_rows && B <= c->ws_batch && T <= c->ws_pos) return 0;      // (ws_pos >= 8192 once allocated)
    if (check_capture) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return lfail("fvhd_llm_prefill: the workspace must grow for this (batch, length) but the stream is being captured - call fvhd_llm_reserve first");
    }
    // the rotary table covers max_position_embeddings (fvhd_llm_set_max_positions; at most 65536 rows = 16 MB at head_dim 64) or 8192
    // positions: position ids of a prefill are < seq_len, and a caller continuing a longer context may pass larger ones - beyond the
    // table the kernel computes the phases itself (llm.hip: rope_kernel), it never clamps
    const int want_pos = c->max_pos > 0 ? (c->max_pos < 65536 ? c->max_pos : 65536) : 8192;
    const int tpos = T > want_pos ? T : want_pos;
    const int nrows = rows > c->ws_rows ? rows : c->ws_rows, nb = B > c->ws_batch ? B : c->ws_batch, np = tpos > c->ws_pos ? tpos : c->ws_pos;
    const int lb = (nb + 15) / 16 * 16;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al256(bytes); return o; };
    const size_t o_h = take((size_t)nrows * c->H * 2), o_xn = take((size_t)nrows * c->H * 2), o_qkv = take((size_t)nrows * c->qkvw * 2),
                 o_att = take((size_t)nrows * c->nh * c->hd * 2), o_act = take((size_t)nrows * c->I * 2), o_last = take((size_t)lb * c->H * 2),
                 o_lastn = take((size_t)lb * c->H * 2), o_rope = take((size_t)np * c->hd * 4),
                 o_part = take((size_t)nrows * std::max(kMaxSplits * c->H, 2 * c->qkvw) * 4);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return lhip("hipDeviceSynchronize", e);
    if (c->ws) {
        if (c->ws_captured) c->retired.push_back(c->ws);      // a caller's graph may still replay on it
        else (void)hipFree(c->ws);
    }
    c->ws = nullptr;
    c->ws_captured = false;
    ++c->generation;
    e = hipMalloc((void**)&c->ws, off);
    if (e != hipSuccess) return lhip("hipMalloc(llm workspace)", e);
    e = hipMemset(c->ws, 0, off);           // the padding rows start (and stay) finite
    if (e != hipSuccess) return lhip("hipMemset(llm workspace)", e);
    c->ws_bytes = off; c->ws_rows = nrows; c->ws_batch = nb; c->ws_pos = np;
    c->h = c->ws + o_h; c->xn = c->ws + o_xn; c->qkv = c->ws + o_qkv; c->att = c->ws + o_att; c->act = c->ws + o_act;
    c->last = c->ws + o_last; c->lastn = c->ws + o_lastn; c->rope = (float*)(c->ws + o_rope); c->part = (float*)(c->ws + o_part);
    // rotary table, fp32 like Qwen2RotaryEmbedding.forward: inv_freq_i = theta^(-2i/hd), angle = pos * inv_freq_i, (cos, sin)
    std::vector<float> tab((size_t)np * c->hd);
    for (int p = 0; p < np; ++p)
        for (int i = 0; i < c->hd / 2; ++i) {
            const float inv = 1.0f / powf(c->theta, (float)(2 * i) / (float)c->hd);
            const float ang = (float)p * inv;
            tab[((size_t)p * (c->hd / 2) + i) * 2] = cosf(ang);
            tab[((size_t)p * (c->hd / 2) + i) * 2 + 1] = sinf(ang);
        }
    e = hipMemcpy(c->rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : lhip("hipMemcpy(rope table)", e);
}

#define LCHECK(expr, what)                                   \
    do {                                                     \
        int _e = (expr);                                     \
        if (_e) return lhip(what, (hipError_t)_e);           \
    } while (0)

}  // namespace

extern "C" {

int fvhd_llm_create(fvhd_llm** out, int device, int hidden, int n_layers, int n_heads, int n_kv_heads, int head_dim, int intermediate,
                    int vocab, float rms_eps, float rope_theta)
{
    if (!out) return lfail("fvhd_llm_create: out is NULL");
    *out = nullptr;
    if (hidden <= 0 || n_layers <= 0 || n_heads <= 0 || n_kv_heads <= 0 || intermediate <= 0 || vocab <= 0)
        return lfail("fvhd_llm_create: sizes must be positive");
    if (head_dim != 64 && head_dim != 128) return lfail("fvhd_llm_create: head_dim must be 64 or 128 (Qwen2-0.5B/1.5B: 64 / 128, 7B: 128)");
    if (n_heads % n_kv_heads) return lfail("fvhd_llm_create: n_heads must be a multiple of n_kv_heads");
    const int qkvw = (n_heads + 2 * n_kv_heads) * head_dim;
    if (hidden % 64 || (n_heads * head_dim) % 64 || intermediate % 64 || qkvw % 16 || vocab % 16)
        return lfail("fvhd_llm_create: hidden, n_heads * head_dim and intermediate must be multiples of 64, vocab of 16");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return lfail("fvhd_llm_create: no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= n) return lfail("fvhd_llm_create: bad device index");
    fvhd_llm* c = new fvhd_llm();
    c->device = device; c->H = hidden; c->L = n_layers; c->nh = n_heads; c->nkv = n_kv_heads; c->hd = head_dim; c->I = intermediate; c->V = vocab;
    c->eps = rms_eps; c->theta = rope_theta; c->qkvw = qkvw;
    if (const char* ev = getenv("FVHD_LLM_SPLITK")) c->down_splits = atoi(ev);      // 0 = never split (A/B)
    if (const char* ev = getenv("FVHD_LLM_OSPLIT")) c->o_splits = atoi(ev);
    if (const char* ev = getenv("FVHD_LLM_QKVSPLIT")) c->qkv_splits = atoi(ev);
    if (const char* ev = getenv("FVHD_LLM_FUSENORM")) c->fuse_norm = atoi(ev);
    if (const char* ev = getenv("FVHD_LLM_FUSEROPE")) c->fuse_rope = atoi(ev);
    if (const char* ev = getenv("FVHD_DEC_RSTD_ONCE")) c->dec_rstd_once = atoi(ev);
    weight_layout(c);
    c->got.assign((size_t)n_layers * 12 + 2, 0);
    DevGuard g(device);
    if (g.err != hipSuccess) { delete c; return lhip("hipSetDevice", g.err); }
    hipError_t e = hipMalloc((void**)&c->wdev, c->wbytes);
    if (e != hipSuccess) { delete c; return lhip("hipMalloc(llm weights)", e); }
    *out = c;
    return 0;
}

void fvhd_llm_destroy(fvhd_llm* c)
{
    if (!c) return;
    DevGuard g(c->device);
    (void)hipDeviceSynchronize();
    if (c->wdev) (void)hipFree(c->wdev);
    if (c->wscratch) (void)hipFree(c->wscratch);
    if (c->ws) (void)hipFree(c->ws);
    for (char* p : c->retired) (void)hipFree(p);
    if (c->load_ev) (void)hipEventDestroy(c->load_ev);
    if (c->emb) (void)hipFree(c->emb);
    if (c->dc) (void)hipFree(c->dc);
    if (c->pre_kv) (void)hipFree(c->pre_kv);
    if (c->status_host) (void)hipHostFree(c->status_host);
    delete c;
}

int fvhd_llm_set_weight_format(fvhd_llm* c, int format)
{
    if (!c) return lfail("fvhd_llm_set_weight_format: ctx is NULL");
    if (format != FVHD_W_BF16 && format != FVHD_W_E4M3) return lfail("fvhd_llm_set_weight_format: format must be FVHD_W_BF16 or FVHD_W_E4M3");
    if (c->any_set)
        return lfail("fvhd_llm_set_weight_format: a tensor was already set - choose the format right after fvhd_llm_create, before the first "
                     "fvhd_llm_set_tensor / fvhd_llm_set_tensor_device (the matrices are quantised as they arrive)");
    if (format == c->wfmt) return 0;
    if (format == FVHD_W_E4M3 && (c->H % 128 || (c->nh * c->hd) % 128 || c->I % 128))
        return lfail("fvhd_llm_set_weight_format: FVHD_W_E4M3 needs hidden, n_heads * head_dim and intermediate to be multiples of 128");
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    if (c->wdev) (void)hipFree(c->wdev);
    if (c->wscratch) (void)hipFree(c->wscratch);
    c->wdev = c->wscratch = nullptr;
    c->wscratch_bytes = 0;
    c->wfmt = format;
    weight_layout(c);
    hipError_t e = hipMalloc((void**)&c->wdev, c->wbytes);
    if (e != hipSuccess) return lhip("hipMalloc(llm weights)", e);
    if (format == FVHD_W_E4M3) {
        const size_t H = c->H, big = std::max(std::max((size_t)c->qkvw, (size_t)2 * c->I), (size_t)c->V) * H;
        c->wscratch_bytes = std::max(big, H * std::max((size_t)c->I, (size_t)c->nh * c->hd)) * 2;
        if ((e = hipMalloc((void**)&c->wscratch, c->wscratch_bytes)) != hipSuccess) return lhip("hipMalloc(dequantisation scratch)", e);
    }
    return 0;
}

int fvhd_llm_weight_bytes(const fvhd_llm* c, size_t* bytes)
{
    if (!c || !bytes) return lfail("fvhd_llm_weight_bytes: NULL argument");
    *bytes = c->wbytes;
    return 0;
}

int fvhd_llm_set_tensor(fvhd_llm* c, const char* key, const void* host_data, int dtype, const int64_t* shape, int ndim)
{
    if (!c || !key || !host_data || !shape) return lfail("fvhd_llm_set_tensor: NULL argument");
    if (dtype < 0 || dtype > 2) return lfail("fvhd_llm_set_tensor: bad dtype");
    if (is_embed_key(key)) {
        if (!(ndim == 2 && shape[0] == c->V && shape[1] == c->H)) return lfail(std::string("fvhd_llm_set_tensor: bad shape for ") + key);
        DevGuard g(c->device);
        if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
        int e = ensure_emb(c);
        if (!e) e = upload_matrix(host_data, dtype, c->V, c->H, c->emb, c->H);
        if (!e) c->any_set = true;
        return e;
    }
    int layer = -1, which = -1;
    const int idx = tensor_index(c, key, &layer, &which);
    if (idx < 0) return lfail(std::string("fvhd_llm_set_tensor: not a tensor of the Qwen2 decoder stack: ") + key);
    const Slot sl = slot_of(c, layer, which);
    const bool vec = sl.cols == 0;
    const bool ok = vec ? (ndim == 1 && (size_t)shape[0] == sl.rows) : (ndim == 2 && (size_t)shape[0] == sl.rows && (size_t)shape[1] == sl.cols);
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    int e = 0;
    if (ok) {
        if (vec) e = upload_vector_f32(host_data, dtype, sl.rows, c->wdev + sl.base + sl.eoff * 4);
        else if (c->wfmt == FVHD_W_E4M3) e = upload_matrix_q(c, host_data, dtype, sl);
        else e = upload_matrix(host_data, dtype, sl.rows, sl.cols, c->wdev + sl.base + sl.eoff * 2, sl.pitch);
    }
    if (!ok) return lfail(std::string("fvhd_llm_set_tensor: bad shape for ") + key);
    if (e) return e;
    c->got[idx] = 1;
    c->any_set = true;
    return 0;
}

// The same tensors from DEVICE memory (a model that already lives on the GPU): matrices bf16, vectors fp32, row-major contiguous, on
// the context's device.  One device-to-device (2-D) copy per tensor on `stream` - no host round trip (advisor, round 3: from_hf moved
// 15 GB of a 7B model through the CPU).  The caller keeps `dev_data` alive until the stream has run the copy.
int fvhd_llm_set_tensor_device(fvhd_llm* c, const char* key, const void* dev_data, int dtype, const int64_t* shape, int ndim, fvhd_stream_t stream)
{
    if (!c || !key || !dev_data || !shape) return lfail("fvhd_llm_set_tensor_device: NULL argument");
    if (is_embed_key(key)) {
        if (!(ndim == 2 && shape[0] == c->V && shape[1] == c->H)) return lfail(std::string("fvhd_llm_set_tensor_device: bad shape for ") + key);
        if (dtype != FVHD_BF16) return lfail("fvhd_llm_set_tensor_device: matrices must be bf16 on the device (model.embed_tokens.weight)");
        DevGuard g(c->device);
        if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
        int e = ensure_emb(c);
        if (e) return e;
        const hipError_t he = hipMemcpyAsync(c->emb, dev_data, (size_t)c->V * c->H * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (he != hipSuccess) return lhip("hipMemcpyAsync(embed_tokens)", he);
        const hipError_t se = hipStreamSynchronize((hipStream_t)stream);     // an optional tensor: no event bookkeeping, the copy is done here
        if (se != hipSuccess) return lhip("hipStreamSynchronize(embed_tokens)", se);
        c->any_set = true;
        return 0;
    }
    int layer = -1, which = -1;
    const int idx = tensor_index(c, key, &layer, &which);
    if (idx < 0) return lfail(std::string("fvhd_llm_set_tensor_device: not a tensor of the Qwen2 decoder stack: ") + key);
    const Slot sl = slot_of(c, layer, which);
    const size_t rows = sl.rows, cols = sl.cols;
    const bool vec = cols == 0;
    if (vec ? !(ndim == 1 && (size_t)shape[0] == rows) : !(ndim == 2 && (size_t)shape[0] == rows && (size_t)shape[1] == cols))
        return lfail(std::string("fvhd_llm_set_tensor_device: bad shape for ") + key);
    if (dtype != (vec ? FVHD_F32 : FVHD_BF16))
        return lfail(std::string("fvhd_llm_set_tensor_device: matrices must be bf16 and vectors fp32 on the device (") + key + ")");
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    hipError_t e = hipSuccess;
    if (vec) e = hipMemcpyAsync(c->wdev + sl.base + sl.eoff * 4, dev_data, rows * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    else if (c->wfmt == FVHD_W_E4M3) {                          // quantised on `stream` straight from the caller's tensor
        if (int qe = quantize_into(c, sl, dev_data, (hipStream_t)stream)) return qe;
    } else
        e = hipMemcpy2DAsync(c->wdev + sl.base + sl.eoff * 2, sl.pitch * 2, dev_data, cols * 2, cols * 2, rows, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return lhip("hipMemcpyAsync(llm weights, device to device)", e);
    // order later work after this copy (advisor, round 4: a prefill on ANOTHER stream could read half-packed weights)
    if (!c->load_ev && (e = hipEventCreateWithFlags(&c->load_ev, hipEventDisableTiming)) != hipSuccess) return lhip("hipEventCreate", e);
    if (c->load_pending && c->load_stream != (hipStream_t)stream) (void)hipEventSynchronize(c->load_ev);   // copies on a second stream: the event follows one stream at a time
    if ((e = hipEventRecord(c->load_ev, (hipStream_t)stream)) != hipSuccess) return lhip("hipEventRecord", e);
    c->load_stream = (hipStream_t)stream;
    c->load_pending = true;
    c->got[idx] = 1;
    c->any_set = true;
    return 0;
}

// every copy fvhd_llm_set_tensor_device has enqueued so far has completed (host wait); the caller holds a DevGuard
static int wait_for_loads(fvhd_llm* c)
{
    if (!c->load_pending) return 0;
    const hipError_t e = hipEventSynchronize(c->load_ev);
    if (e != hipSuccess) return lhip("hipEventSynchronize(llm weights)", e);
    c->load_pending = false;
    return 0;
}

int fvhd_llm_set_max_positions(fvhd_llm* c, int max_position_embeddings)
{
    if (!c || max_position_embeddings <= 0) return lfail("fvhd_llm_set_max_positions: bad argument");
    c->max_pos = max_position_embeddings;      // takes effect at the next workspace (re)allocation: call it before fvhd_llm_reserve
    return 0;
}

int fvhd_llm_workspace_generation(const fvhd_llm* c) { return c ? c->generation : -1; }

int fvhd_llm_finalize(fvhd_llm* c)
{
    if (!c) return lfail("fvhd_llm_finalize: ctx is NULL");
    for (size_t i = 0; i < c->got.size(); ++i)
        if (!c->got[i]) {
            const size_t l = i / 12, w = i % 12;
            return lfail("fvhd_llm_finalize: missing tensor (layer " + std::to_string(l) + ", slot " + std::to_string(w) +
                         "; slots: ln1 q.w q.b k.w k.b v.w v.b o.w ln2 gate up down | norm lm_head)");
        }
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    return wait_for_loads(c);               // the device-to-device packing is complete when this returns (include/fvhd.h "stream contract")
}

int fvhd_llm_reserve(fvhd_llm* c, int batch, int seq_len)
{
    if (!c || batch <= 0 || seq_len <= 0) return lfail("fvhd_llm_reserve: bad argument");
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    return ensure_ws(c, batch, seq_len, nullptr, false);
}

int fvhd_llm_prefill(fvhd_llm* c, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int batch, int seq_len,
                     float* logits_out, void* k_cache, void* v_cache, fvhd_stream_t stream)
{
    if (!c || !embeds || !logits_out) return lfail("fvhd_llm_prefill: NULL argument");
    if (dtype < 0 || dtype > 2) return lfail("fvhd_llm_prefill: bad dtype");
    if (batch <= 0 || seq_len <= 0) return lfail("fvhd_llm_prefill: batch and seq_len must be positive");
    if ((k_cache == nullptr) != (v_cache == nullptr)) return lfail("fvhd_llm_prefill: k_cache and v_cache come together");
    for (char g : c->got)
        if (!g) return lfail("fvhd_llm_prefill: weights incomplete (fvhd_llm_finalize reports the missing tensor)");
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    hipStream_t st = (hipStream_t)stream;
    int e = ensure_ws(c, batch, seq_len, st, true);
    if (e) return e;
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool capturing = hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
        if (capturing) c->ws_captured = true;
        // tensors re-set after fvhd_llm_finalize: this prefill runs behind their copies (a captured stream cannot wait on an outside
        // event - there the host waits once)
        if (c->load_pending) {
            // hipEventQuery / hipEventSynchronize are not capture-safe under the default (global) capture mode: while the caller's stream is
            // capturing they run in relaxed mode, so that they cannot invalidate the caller's capture (round 6, advisor)
            hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
            if (capturing) (void)hipThreadExchangeStreamCaptureMode(&mode);
            const hipError_t q = hipEventQuery(c->load_ev);
            if (q == hipSuccess) c->load_pending = false;
            else if (capturing) e = wait_for_loads(c);
            if (capturing) (void)hipThreadExchangeStreamCaptureMode(&mode);
            if (q != hipSuccess && q != hipErrorNotReady) (void)hipGetLastError();
            if (e) return e;
            if (c->load_pending && !capturing && st != c->load_stream) {
                const hipError_t he = hipStreamWaitEvent(st, c->load_ev, 0);
                if (he != hipSuccess) return lhip("hipStreamWaitEvent(llm weights)", he);
            }
        }
    }
    const int B = batch, T = seq_len, M = B * T, Mp = (M + 255) / 256 * 256;
    const int H = c->H, I = c->I, nh = c->nh, nkv = c->nkv, hd = c->hd;
    const char* w = c->wdev;
    if ((size_t)M * H % 4) return lfail("fvhd_llm_prefill: batch * seq_len * hidden must be a multiple of 4");
    LCHECK(fvhd_launch_cast_rows(st, embeds, dtype, c->h, (long)M * H), "cast embeds");
    const size_t cache_layer = (size_t)B * nkv * T * hd * 2;
    // split-K factor of a GEMM with few output tiles (Mp / 128 x H / 128) - while the tiles of one slice do not fill the chip twice over, K is
    // split across workgroups (fp32 partials + a deterministic reduce that also adds the residual): down_proj 70 -> ~25 us per layer at the
    // 0.5 B prefill shape (B = 8 x 285 tokens).  The reduce of a split GEMM also applies the RMSNorm the next operation starts with
    // (splitk_reduce_norm_kernel, bit-identical to the separate launch): input_layernorm of layer l + 1 behind down_proj of layer l, and -
    // when o_proj is split too (FVHD_LLM_OSPLIT) - post_attention_layernorm behind o_proj
    // the largest split that still fits ONE round of the streaming 128 x 128 kernel (<= 256 workgroups: gemm.hip v1s) - else, as in round 3, the
    // largest within two v1 workgroups per CU.  0.5 B at B = 8 (126 tiles): down_proj in TWO slices of 38 K steps on v1s instead of four of
    // 19 on v1, 33 -> 16 MB of partials: prefill 3.92 -> 3.77 ms (profiles/r04_ttft_down_split.log)
    int ncu_ = 0;
    if (hipDeviceGetAttribute(&ncu_, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || ncu_ <= 0) ncu_ = 256;
    const long ncu = ncu_;
    auto pick_splits = [&](int N, int K, int max_sp) {
        const long tiles = (long)(Mp / 128) * (N / 128);
        if (N % 128 == 0)
            for (long cap = ncu; cap <= 2 * ncu; cap += ncu)        // one round, then two rounds, of one workgroup per CU (256 / 512 on MI355X)
                for (int sp = kMaxSplits; sp > 1; sp >>= 1)
                    if (sp <= max_sp && tiles * sp <= cap && K % (64 * sp) == 0) return sp;
        return 1;
    };
    const int down_sp = pick_splits(H, I, c->down_splits), o_sp = pick_splits(H, nh * hd, c->o_splits);
    // q|k|v projection: split in two, the reduce applies bias + rotary embedding + the KV-cache copies (splitk_bias_rope_kernel)
    const int qkv_sp = pick_splits(c->qkvw, H, std::min(c->qkv_splits, 2));
    // the matrix a GEMM reads: the packed bf16 weights, or - e4m3 - the bf16 scratch the codes are dequantised into right before it
    // (1 byte in, 2 bytes out per element; the GEMMs run one after the other on `st`, so one scratch of the largest matrix serves them all)
    auto weights = [&](size_t off, size_t soff, long N, int K, const void** p) -> int {
        if (c->wfmt != FVHD_W_E4M3) { *p = w + off; return 0; }
        *p = c->wscratch;
        return fvhd_launch_w8_unpack(st, w + off, (const float*)(w + soff), c->wscratch, N, K, 0);
    };
    const void *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wd = nullptr, *wlm = nullptr;
    bool xn_ready = false;                      // c->xn already holds input_layernorm(c->h) of the coming layer
    for (int l = 0; l < c->L; ++l) {
        const LayerOff& o = c->lo[l];
        if (!xn_ready) LCHECK(fvhd_launch_rmsnorm(st, c->h, c->xn, (const float*)(w + o.ln1), Mp, H, c->eps), "rmsnorm 1");
        void* kc = k_cache ? (char*)k_cache + l * cache_layer : nullptr;
        void* vc = v_cache ? (char*)v_cache + l * cache_layer : nullptr;
        LCHECK(weights(o.wqkv, o.sqkv, c->qkvw, H, &wqkv), "dequantise q|k|v");
        if (qkv_sp > 1) {
            LCHECK(fvhd_launch_gemm_splitk_partials(st, c->xn, wqkv, c->part, Mp, c->qkvw, H, qkv_sp), "qkv gemm (split-K)");
            LCHECK(fvhd_launch_splitk_bias_rope(st, c->part, qkv_sp, Mp, (const float*)(w + o.bqkv), c->qkv, (const long*)position_ids, c->rope, kc, vc,
                                                M, T, nh, nkv, hd, c->ws_pos, c->theta), "qkv reduce + bias + rope");
        } else if (c->fuse_rope && fvhd_gemm_qkv_rope_supported(Mp, c->qkvw, H, hd, nh, nkv)) {
            // round 5: bias + rotary embedding + the KV-cache copies in the projection's own epilogue (head_dim 64; bit-identical to the two launches)
            LCHECK(fvhd_launch_gemm_qkv_rope(st, c->xn, wqkv, (const float*)(w + o.bqkv), c->qkv, Mp, c->qkvw, H, (const long*)position_ids, c->rope, kc, vc,
                                             M, T, nh, nkv, hd, c->ws_pos, c->theta), "qkv gemm + rope");
        } else {
            LCHECK(fvhd_launch_gemm(st, c->xn, wqkv, (const float*)(w + o.bqkv), nullptr, nullptr, c->qkv, Mp, c->qkvw, H, EPI_BIAS, FVHD_BF16), "qkv gemm");
            LCHECK(fvhd_launch_rope(st, c->qkv, (const long*)position_ids, c->rope, kc, vc, M, T, nh, nkv, hd, c->ws_pos, c->theta), "rope");
        }
        LCHECK(fvhd_launch_llm_attention(st, c->qkv, c->att, key_valid, B, T, nh, nkv, hd), "attention");
        LCHECK(weights(o.wo, o.so, H, nh * hd, &wo), "dequantise o_proj");
        if (o_sp > 1 && c->fuse_norm) {
            LCHECK(fvhd_launch_gemm_splitk_norm(st, c->att, wo, c->h, c->h, c->part, Mp, H, nh * hd, o_sp, (const float*)(w + o.ln2), c->xn, c->eps),
                   "o_proj gemm (split-K + rmsnorm 2)");
        } else {
            if (o_sp > 1) LCHECK(fvhd_launch_gemm_splitk(st, c->att, wo, c->h, c->h, c->part, Mp, H, nh * hd, o_sp), "o_proj gemm (split-K)");
            else LCHECK(fvhd_launch_gemm(st, c->att, wo, nullptr, nullptr, c->h, c->h, Mp, H, nh * hd, EPI_RESID, FVHD_BF16), "o_proj gemm");
            LCHECK(fvhd_launch_rmsnorm(st, c->h, c->xn, (const float*)(w + o.ln2), Mp, H, c->eps), "rmsnorm 2");
        }
        LCHECK(weights(o.wgu, o.sgu, 2 * (long)I, H, &wgu), "dequantise gate|up");
        LCHECK(fvhd_launch_gemm(st, c->xn, wgu, nullptr, nullptr, nullptr, c->act, Mp, 2 * I, H, EPI_SWIGLU, FVHD_BF16), "gate_up gemm");
        xn_ready = false;
        LCHECK(weights(o.wd, o.sd, H, I, &wd), "dequantise down_proj");
        if (down_sp > 1 && c->fuse_norm && l + 1 < c->L) {
            LCHECK(fvhd_launch_gemm_splitk_norm(st, c->act, wd, c->h, c->h, c->part, Mp, H, I, down_sp, (const float*)(w + c->lo[l + 1].ln1), c->xn, c->eps),
                   "down gemm (split-K + rmsnorm 1 of the next layer)");
            xn_ready = true;
        } else if (down_sp > 1) {
            LCHECK(fvhd_launch_gemm_splitk(st, c->act, wd, c->h, c->h, c->part, Mp, H, I, down_sp), "down gemm (split-K)");
        } else {
            LCHECK(fvhd_launch_gemm(st, c->act, wd, nullptr, nullptr, c->h, c->h, Mp, H, I, EPI_RESID, FVHD_BF16), "down gemm");
        }
    }
    // logits of the LAST position of every sequence (what generate() reads: outputs.logits[:, -1, :])
    LCHECK(fvhd_launch_gather_rows(st, c->h, c->last, B, T, T - 1, H), "gather last rows");
    LCHECK(fvhd_launch_rmsnorm(st, c->last, c->lastn, (const float*)(w + c->norm_off), B, H, c->eps), "final norm");
    LCHECK(weights(c->lm_off, c->lm_soff, c->V, H, &wlm), "dequantise lm_head");
    LCHECK(fvhd_launch_gemm(st, c->lastn, wlm, nullptr, nullptr, nullptr, logits_out, B, c->V, H, EPI_NONE, FVHD_F32), "lm_head gemm");
    return 0;
}

// hidden states after the decoder stack (before the final norm) of the last prefill: [batch * seq_len, hidden] bf16, for tests
int fvhd_llm_debug_hidden(fvhd_llm* c, void* out, int rows, fvhd_stream_t stream)
{
    if (!c || !out || rows <= 0 || rows > c->ws_rows) return lfail("fvhd_llm_debug_hidden: bad argument");
    DevGuard g(c->device);
    hipError_t e = hipMemcpyAsync(out, c->h, (size_t)rows * c->H * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return e == hipSuccess ? 0 : lhip("hipMemcpyAsync", e);
}

// one packed matrix of an e4m3 context in plain [N, K] order (the packing test): codes u8 [N][K], scales fp32 [N], device pointers
int fvhd_llm_debug_packed_e4m3(fvhd_llm* c, int layer, int matrix, void* codes_out, float* scale_out, fvhd_stream_t stream)
{
    if (!c || !codes_out || !scale_out) return lfail("fvhd_llm_debug_packed_e4m3: NULL argument");
    if (c->wfmt != FVHD_W_E4M3) return lfail("fvhd_llm_debug_packed_e4m3: the context holds bf16 weights (fvhd_llm_set_weight_format)");
    if (matrix < FVHD_MAT_QKV || matrix > FVHD_MAT_LM_HEAD || (matrix != FVHD_MAT_LM_HEAD && (layer < 0 || layer >= c->L)))
        return lfail("fvhd_llm_debug_packed_e4m3: matrix must be FVHD_MAT_QKV .. FVHD_MAT_LM_HEAD and layer in [0, n_layers)");
    size_t off = c->lm_off, soff = c->lm_soff;
    long N = c->V;
    int K = c->H;
    if (matrix != FVHD_MAT_LM_HEAD) {
        const LayerOff& o = c->lo[layer];
        switch (matrix) {
        case FVHD_MAT_QKV: off = o.wqkv; soff = o.sqkv; N = c->qkvw; break;
        case FVHD_MAT_O: off = o.wo; soff = o.so; N = c->H; K = c->nh * c->hd; break;
        case FVHD_MAT_GATE_UP: off = o.wgu; soff = o.sgu; N = 2 * (long)c->I; break;
        default: off = o.wd; soff = o.sd; N = c->H; K = c->I; break;
        }
    }
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    if (int e = wait_for_loads(c)) return e;
    LCHECK(fvhd_launch_w8_unpack((hipStream_t)stream, c->wdev + off, nullptr, codes_out, N, K, 1), "fvhd_llm_debug_packed_e4m3");
    const hipError_t he = hipMemcpyAsync(scale_out, c->wdev + soff, (size_t)N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return he == hipSuccess ? 0 : lhip("hipMemcpyAsync", he);
}

// ---- decode: the library's own KV cache, one token per sequence per step (include/fvhd.h "LLM decode") ----
}  // extern "C"

namespace {

fvhd_llm::Plan dec_plan(int N, int K, int ncu)
{
    // split K until the grid holds about two workgroups per CU (at most 16 slices: the last arriver reads them all)
    const int ntiles = N / 16, ncol = (ntiles + 3) / 4, KC = K / 128;
    const int want = (2 * ncu + ncol - 1) / ncol;
    fvhd_llm::Plan p;
    p.S = std::max(1, std::min(std::min(want, KC), 16));
    p.cpw = (KC + p.S - 1) / p.S;
    p.S = (KC + p.cpw - 1) / p.cpw;
    return p;
}

void att_plan(int cap, int heads, int ncu, int* S, int* chunk)
{
    // key slices until the grid (batch * n_heads * slices) holds ~2 workgroups per CU - at B = 1 the 14 heads of Qwen2-0.5B alone fill
    // 14 of 256 CUs - with at least 64 keys (one block per lane) per slice and at most 32 slices
    const int want = (2 * ncu + heads - 1) / heads;
    const int s = std::max(1, std::min(std::min(want, (cap + 63) / 64), 32));
    *chunk = ((cap + s - 1) / s + 63) / 64 * 64;
    *S = (cap + *chunk - 1) / *chunk;
}

int dec_status_error(const fvhd_llm* c, const char* who)
{
    const int st = *(volatile int*)c->status_host;
    if (st == 1)
        return lfail(std::string(who) + ": the KV cache is full (capacity " + std::to_string(c->dc_cap) +
                     " positions): a decode step past it wrote nothing - reserve a larger cache (fvhd_llm_cache_reserve) and start again");
    if (st == 2) return lfail(std::string(who) + ": a decode step was given a token id outside [0, vocab); it wrote nothing - start again");
    return 0;
}

DecSampleArgs dec_sample_args(const fvhd_llm* c, const float* logits, int B)
{
    DecSampleArgs a;
    a.logits = logits; a.B = B; a.V = c->V; a.temperature = c->temperature; a.top_k = c->top_k; a.top_p = c->top_p; a.seed = c->seed;
    return a;
}

const char* sampling_error(float temperature, int top_k, float top_p)
{
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return "temperature must be finite and > 0";
    if (top_k < 0) return "top_k must be >= 0 (0 = off)";
    if (!(top_p >= 0.f && top_p <= 1.f)) return "top_p must be in [0, 1] (1 = off)";
    return nullptr;
}

// the decode's input embedding: model.embed_tokens.weight when it was set, the packed lm_head rows only when the caller said the model ties them
int dec_embedding_error(const fvhd_llm* c, const char* who)
{
    if (c->emb || c->tied == 1) return 0;
    if (c->tied == 0)
        return lfail(std::string(who) + ": this model does not tie its embeddings - set model.embed_tokens.weight (fvhd_llm_set_tensor) before decoding");
    return lfail(std::string(who) + ": the decode's input embedding is unknown - set model.embed_tokens.weight (fvhd_llm_set_tensor), or call "
                 "fvhd_llm_set_tied_embeddings(ctx, 1) for a model whose lm_head IS its embedding table (tie_word_embeddings)");
}

}  // namespace

extern "C" {

int fvhd_llm_set_tied_embeddings(fvhd_llm* c, int tied)
{
    if (!c) return lfail("fvhd_llm_set_tied_embeddings: ctx is NULL");
    c->tied = tied != 0 ? 1 : 0;
    return 0;
}

int fvhd_llm_cache_reserve(fvhd_llm* c, int batch, int capacity)
{
    if (!c || batch < 1 || batch > 64 || capacity < 1) return lfail("fvhd_llm_cache_reserve: needs a context, 1 <= batch <= 64 and capacity >= 1");
    for (char g : c->got)
        if (!g) return lfail("fvhd_llm_cache_reserve: weights incomplete (fvhd_llm_finalize reports the missing tensor)");
    if (c->H % 128 || (c->nh * c->hd) % 128 || c->I % 128)
        return lfail("fvhd_llm_cache_reserve: the decode needs hidden, n_heads * head_dim and intermediate to be multiples of 128");
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    int e = ensure_ws(c, batch, 1, nullptr, false);              // the rotary table
    if (e) return e;
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || ncu <= 0) ncu = 256;
    const int H = c->H, I = c->I, nh = c->nh, nkv = c->nkv, hd = c->hd, V = c->V, L = c->L;
    c->p_qkv = dec_plan(c->qkvw, H, ncu);
    c->p_o = dec_plan(H, nh * hd, ncu);
    c->p_gu = dec_plan(2 * I, H, ncu);
    c->p_d = dec_plan(H, I, ncu);
    c->p_lm = fvhd_llm::Plan{1, H / 128};
    att_plan(capacity, batch * nh, ncu, &c->att_S, &c->att_chunk);
    const int NB = (batch + 15) / 16;                            // batch tiles of the decode GEMM: slabs and (max, index) pairs per tile
    size_t part = 0;
    int ncol = 1;
    for (auto pr : {std::make_pair(c->p_qkv, c->qkvw), std::make_pair(c->p_o, H), std::make_pair(c->p_gu, 2 * I), std::make_pair(c->p_d, H)}) {
        if (pr.first.S > 1) part = std::max(part, (size_t)pr.first.S * pr.second * 64 * NB);
        ncol = std::max(ncol, (pr.second / 16 + 3) / 4);
    }
    const int lm_ncol = (V / 16 + 3) / 4;
    c->cnt_att = ncol;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al256(bytes); return o; };
    const size_t kvb = (size_t)L * batch * nkv * capacity * hd * 2;
    const size_t o_k = take(kvb), o_v = take(kvb), o_mask = take((size_t)batch * capacity), o_pos = take(8 * batch), o_last = take(8 * batch),
                 o_len = take(4), o_status = take(4), o_h = take((size_t)batch * H * 2), o_q = take((size_t)batch * nh * hd * 2),
                 o_att = take((size_t)batch * nh * hd * 2), o_act = take((size_t)batch * I * 2), o_part = take(std::max(part, (size_t)16)),
                 o_apart = take((size_t)batch * nh * c->att_S * (hd + 2) * 4), o_cnt = take((size_t)(ncol + batch * nh) * 4),
                 o_av = take((size_t)lm_ncol * 16 * NB * 4), o_ai = take((size_t)lm_ncol * 16 * NB * 4), o_logits = take((size_t)batch * V * 4),
                 o_rope = take((size_t)c->ws_pos * hd * 4), o_sws = take(fvhd_dec_sample_ws_bytes()), o_rstd = take(4 * 64);
    hipError_t he = hipDeviceSynchronize();                      // refused while a stream is being captured (like fvhd_llm_reserve)
    if (he != hipSuccess) return lhip("fvhd_llm_cache_reserve: hipDeviceSynchronize", he);
    if (c->dc) (void)hipFree(c->dc);
    c->dc = nullptr;
    c->dc_batch = c->dc_cap = c->run_batch = 0;
    if ((he = hipMalloc((void**)&c->dc, off)) != hipSuccess) return lhip("hipMalloc(llm KV cache)", he);
    if ((he = hipMemset(c->dc, 0, off)) != hipSuccess) return lhip("hipMemset(llm KV cache)", he);      // counters start at zero
    if (!c->status_host) {
        if ((he = hipHostMalloc((void**)&c->status_host, 4, hipHostMallocMapped)) != hipSuccess) return lhip("hipHostMalloc(status word)", he);
        if ((he = hipHostGetDevicePointer((void**)&c->status_host_dev, c->status_host, 0)) != hipSuccess) return lhip("hipHostGetDevicePointer", he);
    }
    *(volatile int*)c->status_host = 0;
    char* d = c->dc;
    c->kcache = d + o_k; c->vcache = d + o_v; c->mask = (unsigned char*)(d + o_mask); c->posv = (int64_t*)(d + o_pos); c->last_ids = (int64_t*)(d + o_last);
    c->len = (int*)(d + o_len); c->status = (int*)(d + o_status); c->dh = d + o_h; c->dq = d + o_q; c->datt = d + o_att; c->dact = d + o_act;
    c->dpart = (float*)(d + o_part); c->apart = (float*)(d + o_apart); c->cnt = (int*)(d + o_cnt); c->amax_v = (float*)(d + o_av);
    c->amax_i = (int*)(d + o_ai); c->dlogits = (float*)(d + o_logits); c->drope = (float*)(d + o_rope); c->sws = d + o_sws; c->drstd = (float*)(d + o_rstd);
    c->dc_bytes = off; c->dc_batch = batch; c->dc_cap = capacity; c->dc_pos = c->ws_pos;
    // the decode's own copy of the rotary table: a later, larger prefill may replace the prefill workspace under a captured decode graph
    if ((he = hipMemcpy(c->drope, c->rope, (size_t)c->ws_pos * hd * 4, hipMemcpyDeviceToDevice)) != hipSuccess) return lhip("hipMemcpy(rope table)", he);
    return 0;
}

int fvhd_llm_start(fvhd_llm* c, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int batch, int seq_len,
                   float* logits_out, int64_t* next_ids_out, fvhd_stream_t stream)
{
    if (!c || !embeds) return lfail("fvhd_llm_start: NULL argument");
    if (!c->dc) return lfail("fvhd_llm_start: no KV cache - call fvhd_llm_cache_reserve first");
    if (batch < 1 || batch > c->dc_batch) return lfail("fvhd_llm_start: batch must be in [1, the batch of fvhd_llm_cache_reserve]");
    if (seq_len < 1 || seq_len > c->dc_cap) return lfail("fvhd_llm_start: seq_len must be in [1, the capacity of fvhd_llm_cache_reserve]");
    if (int e = dec_embedding_error(c, "fvhd_llm_start")) return e;
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    hipStream_t st = (hipStream_t)stream;
    const int L = c->L, nkv = c->nkv, hd = c->hd, T = seq_len, B = batch, cap = c->dc_cap;
    const size_t layer_src = (size_t)B * nkv * T * hd * 2, need = 2 * (size_t)L * layer_src;
    if (need > c->pre_kv_bytes) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return lfail("fvhd_llm_start: its staging buffer must grow but the stream is being captured");
        hipError_t he = hipDeviceSynchronize();
        if (he != hipSuccess) return lhip("hipDeviceSynchronize", he);
        if (c->pre_kv) (void)hipFree(c->pre_kv);
        c->pre_kv = nullptr;
        c->pre_kv_bytes = 0;
        if ((he = hipMalloc((void**)&c->pre_kv, need)) != hipSuccess) return lhip("hipMalloc(prefill KV staging)", he);
        c->pre_kv_bytes = need;
    }
    *(volatile int*)c->status_host = 0;
    float* logits = logits_out ? logits_out : c->dlogits;
    char* pk = c->pre_kv;
    char* pv = c->pre_kv + (size_t)L * layer_src;
    int e = fvhd_llm_prefill(c, embeds, dtype, key_valid, position_ids, B, T, logits, pk, pv, stream);
    if (e) return e;
    const size_t layer_dst = (size_t)c->dc_batch * nkv * cap * hd * 2;
    for (int l = 0; l < L; ++l) {
        hipError_t he = hipMemcpy2DAsync(c->kcache + l * layer_dst, (size_t)cap * hd * 2, pk + l * layer_src, (size_t)T * hd * 2, (size_t)T * hd * 2,
                                         (size_t)B * nkv, hipMemcpyDeviceToDevice, st);
        if (he == hipSuccess)
            he = hipMemcpy2DAsync(c->vcache + l * layer_dst, (size_t)cap * hd * 2, pv + l * layer_src, (size_t)T * hd * 2, (size_t)T * hd * 2,
                                  (size_t)B * nkv, hipMemcpyDeviceToDevice, st);
        if (he != hipSuccess) return lhip("hipMemcpy2DAsync(KV cache)", he);
    }
    hipError_t he = hipMemsetAsync(c->mask, 0, (size_t)c->dc_batch * cap, st);
    if (he == hipSuccess)
        he = key_valid ? hipMemcpy2DAsync(c->mask, cap, key_valid, T, T, B, hipMemcpyDeviceToDevice, st) : hipMemset2DAsync(c->mask, cap, 1, T, B, st);
    if (he != hipSuccess) return lhip("key mask copy", he);
    if (c->do_sample) {
        // sampling: the cache state first, so that the draw reads n = the prompt length from the device
        LCHECK(fvhd_launch_dec_start_state(st, c->posv, position_ids, B, T, c->len, c->status), "decode state");
        DecSampleArgs a = dec_sample_args(c, logits, B);
        a.len = c->len;
        a.last = c->last_ids;
        a.ids_out = next_ids_out;
        LCHECK(fvhd_launch_dec_sample(st, &a, c->sws), "first-token sampling");
        c->run_batch = B;
        return 0;
    }
    // the first token: the same (max, index) pairs + reduce as the decode's lm_head (lowest index on ties), then the cache state
    LCHECK(fvhd_launch_dec_argmax_blocks(st, logits, c->V, B, c->amax_v, c->amax_i), "first-token argmax (blocks)");
    LCHECK(fvhd_launch_dec_argmax_finish(st, c->amax_v, c->amax_i, (c->V + 63) / 64, B, c->last_ids, next_ids_out, nullptr, nullptr, nullptr),
           "first-token argmax (reduce)");
    LCHECK(fvhd_launch_dec_start_state(st, c->posv, position_ids, B, T, c->len, c->status), "decode state");
    c->run_batch = B;
    return 0;
}

int fvhd_llm_decode(fvhd_llm* c, const int64_t* token_ids, float* logits_out, int64_t* next_ids_out, fvhd_stream_t stream)
{
    if (!c) return lfail("fvhd_llm_decode: ctx is NULL");
    if (!c->dc || !c->run_batch) return lfail("fvhd_llm_decode: no started sequence - call fvhd_llm_cache_reserve and fvhd_llm_start first");
    if (int e = dec_status_error(c, "fvhd_llm_decode")) return e;
    if (int e = dec_embedding_error(c, "fvhd_llm_decode")) return e;
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    hipStream_t st = (hipStream_t)stream;
    const int B = c->run_batch, H = c->H, I = c->I, nh = c->nh, nkv = c->nkv, hd = c->hd, cap = c->dc_cap;
    const char* w = c->wdev;
    const bool q8 = c->wfmt == FVHD_W_E4M3;
    if (q8 && !c->emb) {                                         // a tied model: the token row dequantised from the lm_head codes
        LCHECK(fvhd_launch_dec_embed_w8(st, token_ids, c->last_ids, w + c->lm_off, (const float*)(w + c->lm_soff), c->V, H, c->dh, c->mask, B, cap, c->len,
                                        c->status, c->status_host_dev), "decode embed (e4m3 lm_head rows)");
    } else {
        LCHECK(fvhd_launch_dec_embed(st, token_ids, c->last_ids, c->emb ? c->emb : w + c->lm_off, c->V, H, c->dh, c->mask, B, cap, c->len, c->status,
                                     c->status_host_dev), "decode embed");
    }
    const size_t layer_kv = (size_t)c->dc_batch * nkv * cap * hd * 2;
    auto gemm = [&](int epi, const void* x, int K, const float* norm_w, const void* W, size_t soff, int N, const fvhd_llm::Plan& p) {
        DecGemmArgs a;
        a.wscale = q8 ? (const float*)(w + soff) : nullptr;
        a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = c->eps; a.W = W; a.N = N; a.K = K; a.B = B; a.S = p.S; a.cpw = p.cpw;
        a.part = c->dpart; a.cnt = c->cnt; a.epi = epi; a.status = c->status; a.rstd = c->dec_rstd_once ? c->drstd : nullptr;
        return a;
    };
    for (int l = 0; l < c->L; ++l) {
        const LayerOff& o = c->lo[l];
        DecGemmArgs a = gemm(DEC_EPI_QKV, c->dh, H, (const float*)(w + o.ln1), w + o.wqkv, o.sqkv, c->qkvw, c->p_qkv);
        a.bias = (const float*)(w + o.bqkv); a.out = c->dq; a.ldo = nh * hd; a.pos = c->posv; a.rope = c->drope; a.P = c->dc_pos; a.theta = c->theta;
        a.nh = nh; a.nkv = nkv; a.hd = hd; a.kc = c->kcache + l * layer_kv; a.vc = c->vcache + l * layer_kv; a.cap = cap; a.len = c->len;
        LCHECK(fvhd_launch_dec_gemm(st, &a), "decode q|k|v + rope + cache append");
        LCHECK(fvhd_launch_dec_attention(st, c->dq, c->kcache + l * layer_kv, c->vcache + l * layer_kv, c->mask, c->datt, B, nh, nkv, hd, cap, c->len, 1,
                                         c->att_S, c->att_chunk, c->apart, c->cnt + c->cnt_att, c->status), "decode attention");
        a = gemm(DEC_EPI_RESID, c->datt, nh * hd, nullptr, w + o.wo, o.so, H, c->p_o);
        a.resid = c->dh; a.out = c->dh; a.ldo = H;
        LCHECK(fvhd_launch_dec_gemm(st, &a), "decode o_proj + residual");
        a = gemm(DEC_EPI_SWIGLU, c->dh, H, (const float*)(w + o.ln2), w + o.wgu, o.sgu, 2 * I, c->p_gu);
        a.out = c->dact; a.ldo = I;
        LCHECK(fvhd_launch_dec_gemm(st, &a), "decode rmsnorm + gate|up + silu");
        a = gemm(DEC_EPI_RESID, c->dact, I, nullptr, w + o.wd, o.sd, H, c->p_d);
        a.resid = c->dh; a.out = c->dh; a.ldo = H;
        LCHECK(fvhd_launch_dec_gemm(st, &a), "decode down_proj + residual");
    }
    DecGemmArgs a = gemm(DEC_EPI_ARGMAX, c->dh, H, (const float*)(w + c->norm_off), w + c->lm_off, c->lm_soff, c->V, c->p_lm);
    a.logits = logits_out; a.amax_v = c->amax_v; a.amax_i = c->amax_i;
    if (c->do_sample) {
        // sampling replaces the argmax reduce: it reads the logits (the caller's, else the context's buffer), chooses with n = length + 1
        // (the cache holds this step's token), and advances positions and length
        if (!a.logits) a.logits = c->dlogits;
        LCHECK(fvhd_launch_dec_gemm(st, &a), "decode final norm + lm_head");
        DecSampleArgs sa = dec_sample_args(c, a.logits, B);
        sa.len = c->len; sa.n_add = 1; sa.last = c->last_ids; sa.ids_out = next_ids_out; sa.posv = c->posv; sa.len_advance = c->len;
        sa.status = c->status;
        LCHECK(fvhd_launch_dec_sample(st, &sa, c->sws), "decode sampling");
        return 0;
    }
    LCHECK(fvhd_launch_dec_gemm(st, &a), "decode final norm + lm_head + argmax");
    LCHECK(fvhd_launch_dec_argmax_finish(st, c->amax_v, c->amax_i, (c->V / 16 + 3) / 4, B, c->last_ids, next_ids_out, c->posv, c->len, c->status),
           "decode argmax reduce");
    return 0;
}

int fvhd_llm_set_sampling(fvhd_llm* c, int do_sample, float temperature, int top_k, float top_p, unsigned long long seed)
{
    if (!c) return lfail("fvhd_llm_set_sampling: ctx is NULL");
    if (const char* e = sampling_error(temperature, top_k, top_p)) return lfail(std::string("fvhd_llm_set_sampling: ") + e);
    c->do_sample = do_sample != 0;
    c->temperature = temperature;
    c->top_k = top_k;
    c->top_p = top_p;
    c->seed = seed;
    return 0;
}

int fvhd_llm_cache_state(fvhd_llm* c, int* length, int* status)
{
    if (!c || !c->dc) return lfail("fvhd_llm_cache_state: no KV cache");
    DevGuard g(c->device);
    if (g.err != hipSuccess) return lhip("hipSetDevice", g.err);
    int v[2] = {0, 0};
    hipError_t he = hipDeviceSynchronize();
    if (he == hipSuccess) he = hipMemcpy(&v[0], c->len, 4, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(&v[1], c->status, 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return lhip("fvhd_llm_cache_state", he);
    if (length) *length = v[0];
    if (status) *status = v[1];
    return 0;
}

// ---- single ops (unit tests) ----
int fvhd_op_rmsnorm(fvhd_stream_t st, const void* x, void* y, const float* w, int M, int H, float eps)
{
    if (!x || !y || !w) return lfail("fvhd_op_rmsnorm: NULL pointer");
    int e = fvhd_launch_rmsnorm((hipStream_t)st, x, y, w, M, H, eps);
    return e ? lhip("fvhd_op_rmsnorm", (hipError_t)e) : 0;
}

int fvhd_op_rope(fvhd_stream_t st, void* qkv, const int64_t* pos, const float* table, void* k_cache, void* v_cache, int M, int T, int n_heads,
                 int n_kv_heads, int head_dim, int table_positions, float rope_theta)
{
    if (!qkv || !table) return lfail("fvhd_op_rope: NULL pointer");
    int e = fvhd_launch_rope((hipStream_t)st, qkv, (const long*)pos, table, k_cache, v_cache, M, T, n_heads, n_kv_heads, head_dim, table_positions, rope_theta);
    return e ? lhip("fvhd_op_rope", (hipError_t)e) : 0;
}

int fvhd_op_gemm_qkv_rope(fvhd_stream_t st, const void* A, const void* Wt, const float* bias, void* out, int Mp, int N, int K, const int64_t* pos,
                          const float* table, void* k_cache, void* v_cache, int M, int T, int n_heads, int n_kv_heads, int head_dim, int table_positions,
                          float rope_theta)
{
    if (!A || !Wt || !bias || !out || !table) return lfail("fvhd_op_gemm_qkv_rope: NULL pointer");
    if (!fvhd_gemm_qkv_rope_supported(Mp, N, K, head_dim, n_heads, n_kv_heads))
        return lfail("fvhd_op_gemm_qkv_rope: needs head_dim 64, N = (n_heads + 2 n_kv_heads) * 64, Mp % 128 == 0, N % 128 == 0, K % 64 == 0 and at most one "
                     "128 x 128 tile per CU (fvhd_gemm_qkv_rope_supported); other shapes run fvhd_op_gemm + fvhd_op_rope");
    int e = fvhd_launch_gemm_qkv_rope((hipStream_t)st, A, Wt, bias, out, Mp, N, K, (const long*)pos, table, k_cache, v_cache, M, T, n_heads, n_kv_heads,
                                      head_dim, table_positions, rope_theta);
    return e ? lhip("fvhd_op_gemm_qkv_rope", (hipError_t)e) : 0;
}

int fvhd_op_gemm_splitk(fvhd_stream_t st, const void* A, const void* Wt, const void* resid, void* out, float* partial, int M, int N, int K, int splits)
{
    if (!A || !Wt || !out || !partial) return lfail("fvhd_op_gemm_splitk: NULL pointer");
    if (splits < 1 || N % 128 || K % (64 * splits)) return lfail("fvhd_op_gemm_splitk: needs N % 128 == 0 and K % (64 * splits) == 0");
    int e = fvhd_launch_gemm_splitk((hipStream_t)st, A, Wt, resid, out, partial, M, N, K, splits);
    return e ? lhip("fvhd_op_gemm_splitk", (hipError_t)e) : 0;
}

int fvhd_op_gemm_splitk_norm(fvhd_stream_t st, const void* A, const void* Wt, const void* resid, void* out, float* partial, int M, int N, int K, int splits,
                             const float* norm_w, void* norm_out, float eps)
{
    if (!A || !Wt || !out || !partial || !norm_w || !norm_out) return lfail("fvhd_op_gemm_splitk_norm: NULL pointer");
    if (norm_out == out) return lfail("fvhd_op_gemm_splitk_norm: norm_out must not alias out");
    if (splits < 1 || N % 128 || K % (64 * splits)) return lfail("fvhd_op_gemm_splitk_norm: needs N % 128 == 0 and K % (64 * splits) == 0");
    int e = fvhd_launch_gemm_splitk_norm((hipStream_t)st, A, Wt, resid, out, partial, M, N, K, splits, norm_w, norm_out, eps);
    return e ? lhip("fvhd_op_gemm_splitk_norm", (hipError_t)e) : 0;
}

int fvhd_op_qkv_splitk_rope(fvhd_stream_t st, const void* A, const void* Wt, const float* bias, float* partial, void* qkv, const int64_t* pos,
                            const float* table, void* k_cache, void* v_cache, int M, int Mp, int K, int T, int n_heads, int n_kv_heads, int head_dim,
                            int table_positions, float rope_theta, int splits)
{
    if (!A || !Wt || !partial || !qkv || !table) return lfail("fvhd_op_qkv_splitk_rope: NULL pointer");
    const int width = (n_heads + 2 * n_kv_heads) * head_dim;
    if (splits < 1 || width % 128 || K % (64 * splits) || Mp < M) return lfail("fvhd_op_qkv_splitk_rope: needs width % 128 == 0, K % (64 * splits) == 0, Mp >= M");
    int e = fvhd_launch_gemm_splitk_partials((hipStream_t)st, A, Wt, partial, Mp, width, K, splits);
    if (e) return lhip("fvhd_op_qkv_splitk_rope (gemm)", (hipError_t)e);
    e = fvhd_launch_splitk_bias_rope((hipStream_t)st, partial, splits, Mp, bias, qkv, (const long*)pos, table, k_cache, v_cache, M, T, n_heads, n_kv_heads,
                                     head_dim, table_positions, rope_theta);
    return e ? lhip("fvhd_op_qkv_splitk_rope (reduce)", (hipError_t)e) : 0;
}

int fvhd_op_attention_causal(fvhd_stream_t st, const void* qkv, void* out, const uint8_t* key_valid, int B, int T, int n_heads, int n_kv_heads, int head_dim)
{
    if (!qkv || !out) return lfail("fvhd_op_attention_causal: NULL pointer");
    int e = fvhd_launch_llm_attention((hipStream_t)st, qkv, out, key_valid, B, T, n_heads, n_kv_heads, head_dim);
    return e ? lhip("fvhd_op_attention_causal", (hipError_t)e) : 0;
}

// ---- single ops of the decode step (unit tests) ----
static void dec_split(DecGemmArgs& a, int splits)
{
    a.cpw = (a.K / 128 + splits - 1) / splits;
    a.S = (a.K / 128 + a.cpw - 1) / a.cpw;
}

int fvhd_op_dec_gemm(fvhd_stream_t st, int epi, const void* x, int B, const float* norm_w, float eps, const void* Wt, int N, int K, const void* resid,
                     void* out, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !out || (epi == FVHD_EPI_RESID && !resid)) return lfail("fvhd_op_dec_gemm: NULL pointer");
    if (epi != FVHD_EPI_RESID && epi != FVHD_EPI_SWIGLU) return lfail("fvhd_op_dec_gemm: epi must be FVHD_EPI_RESID or FVHD_EPI_SWIGLU");
    if (B < 1 || B > 64 || N % 16 || K % 128 || splits < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_gemm: needs 1 <= B <= 64, N % 16 == 0, K % 128 == 0, splits >= 1 (and scratch when splits > 1)");
    DecGemmArgs a;
    a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = eps; a.W = Wt; a.N = N; a.K = K; a.B = B; a.part = partial; a.cnt = counters;
    a.epi = epi; a.resid = resid; a.out = out; a.ldo = epi == FVHD_EPI_SWIGLU ? N / 2 : N;
    dec_split(a, splits);
    int e = fvhd_launch_dec_gemm((hipStream_t)st, &a);
    return e ? lhip("fvhd_op_dec_gemm", (hipError_t)e) : 0;
}

int fvhd_op_dec_qkv(fvhd_stream_t st, const void* x, int B, int K, const float* norm_w, float eps, const void* Wt, const float* bias, void* q_out,
                    const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache, void* v_cache, int capacity,
                    const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !bias || !q_out || !pos || !table || !k_cache || !v_cache || !length) return lfail("fvhd_op_dec_qkv: NULL pointer");
    if (B < 1 || B > 64 || K % 128 || splits < 1 || head_dim % 16 || n_heads < 1 || n_kv_heads < 1 || capacity < 1 || table_positions < 1 ||
        (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_qkv: needs 1 <= B <= 64, K % 128 == 0, head_dim % 16 == 0, splits >= 1 (and scratch when splits > 1)");
    DecGemmArgs a;
    a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = eps; a.W = Wt; a.N = (n_heads + 2 * n_kv_heads) * head_dim; a.K = K; a.B = B;
    a.part = partial; a.cnt = counters; a.epi = DEC_EPI_QKV; a.bias = bias; a.out = q_out; a.ldo = n_heads * head_dim; a.pos = pos; a.rope = table;
    a.P = table_positions; a.theta = rope_theta; a.nh = n_heads; a.nkv = n_kv_heads; a.hd = head_dim; a.kc = k_cache; a.vc = v_cache; a.cap = capacity;
    a.len = length;
    dec_split(a, splits);
    int e = fvhd_launch_dec_gemm((hipStream_t)st, &a);
    return e ? lhip("fvhd_op_dec_qkv", (hipError_t)e) : 0;
}

int fvhd_op_dec_attention(fvhd_stream_t st, const void* q, const void* k_cache, const void* v_cache, const uint8_t* key_valid, void* out, int B, int n_heads,
                          int n_kv_heads, int head_dim, int capacity, const int* length, float* partial, int* counters, int splits)
{
    if (!q || !k_cache || !v_cache || !key_valid || !out || !length) return lfail("fvhd_op_dec_attention: NULL pointer");
    if (B < 1 || B > 64) return lfail("fvhd_op_dec_attention: needs 1 <= B <= 64");
    if (splits < 1 || capacity < 1 || (splits > 1 && (!partial || !counters))) return lfail("fvhd_op_dec_attention: splits >= 1 (and scratch when splits > 1)");
    const int chunk = ((capacity + splits - 1) / splits + 63) / 64 * 64, S = (capacity + chunk - 1) / chunk;
    int e = fvhd_launch_dec_attention((hipStream_t)st, q, k_cache, v_cache, key_valid, out, B, n_heads, n_kv_heads, head_dim, capacity, length, 0, S, chunk,
                                      partial, counters, nullptr);
    return e ? lhip("fvhd_op_dec_attention", (hipError_t)e) : 0;
}

int fvhd_op_dec_lm_argmax(fvhd_stream_t st, const void* x, int B, const float* norm_w, float eps, const void* Wt, int V, int K, float* logits, int64_t* ids_out,
                          float* scratch_v, int* scratch_i)
{
    if (!x || !Wt || !ids_out || !scratch_v || !scratch_i) return lfail("fvhd_op_dec_lm_argmax: NULL pointer");
    if (B < 1 || B > 64 || V % 16 || K % 128) return lfail("fvhd_op_dec_lm_argmax: needs 1 <= B <= 64, V % 16 == 0, K % 128 == 0");
    DecGemmArgs a;
    a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = eps; a.W = Wt; a.N = V; a.K = K; a.B = B; a.S = 1; a.cpw = K / 128; a.epi = DEC_EPI_ARGMAX;
    a.logits = logits; a.amax_v = scratch_v; a.amax_i = scratch_i;
    int e = fvhd_launch_dec_gemm((hipStream_t)st, &a);
    if (!e) e = fvhd_launch_dec_argmax_finish((hipStream_t)st, scratch_v, scratch_i, (V / 16 + 3) / 4, B, nullptr, ids_out, nullptr, nullptr, nullptr);
    return e ? lhip("fvhd_op_dec_lm_argmax", (hipError_t)e) : 0;
}

// ---- the same single ops on e4m3 weights: Wt = plain row-major codes u8 [N][K], scale fp32 [N] ----
// The kernels read the packed K order (llm_w8.hip): the codes are repacked into a process-wide scratch first, grown on demand - eager
// calls only, like fvhd_op_dec_sample's workspace.
static int w8_op_repack(hipStream_t st, const char* who, const void* Wt, long N, int K, const void** packed)
{
    static char* buf[64] = {};
    static size_t cap[64] = {};
    int dev = 0;
    hipError_t he = hipGetDevice(&dev);
    if (he != hipSuccess) return lhip("hipGetDevice", he);
    if (dev < 0 || dev >= 64) return lfail(std::string(who) + ": device index out of range");
    const size_t need = (size_t)N * K;
    if (need > cap[dev]) {
        if (buf[dev]) (void)hipFree(buf[dev]);                  // (synchronises: no earlier launch still reads it)
        buf[dev] = nullptr;
        cap[dev] = 0;
        if ((he = hipMalloc((void**)&buf[dev], need)) != hipSuccess) { buf[dev] = nullptr; return lhip("hipMalloc(e4m3 repack scratch)", he); }
        cap[dev] = need;
    }
    const int e = fvhd_launch_w8_unpack(st, Wt, nullptr, buf[dev], N, K, 2);
    if (e) return lhip(who, (hipError_t)e);
    *packed = buf[dev];
    return 0;
}

int fvhd_op_quantize_e4m3(fvhd_stream_t st, const void* W, int N, int K, void* codes, float* scale)
{
    if (!W || !codes || !scale) return lfail("fvhd_op_quantize_e4m3: NULL pointer");
    if (N < 1 || K < 8 || K % 8) return lfail("fvhd_op_quantize_e4m3: needs N >= 1, K >= 8 and K % 8 == 0");
    int e = fvhd_launch_quantize_e4m3((hipStream_t)st, W, N, K, codes, K, scale, 1, 0);
    return e ? lhip("fvhd_op_quantize_e4m3", (hipError_t)e) : 0;
}

int fvhd_op_dec_gemm_w8(fvhd_stream_t st, int epi, const void* x, int B, const float* norm_w, float eps, const void* Wt, const float* scale, int N, int K,
                        const void* resid, void* out, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !scale || !out || (epi == FVHD_EPI_RESID && !resid)) return lfail("fvhd_op_dec_gemm_w8: NULL pointer");
    if (epi != FVHD_EPI_RESID && epi != FVHD_EPI_SWIGLU) return lfail("fvhd_op_dec_gemm_w8: epi must be FVHD_EPI_RESID or FVHD_EPI_SWIGLU");
    if (B < 1 || B > 64 || N < 16 || N % 16 || K < 128 || K % 128 || splits < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_gemm_w8: needs 1 <= B <= 64, N % 16 == 0, K % 128 == 0, splits >= 1 (and scratch when splits > 1)");
    DecGemmArgs a;
    if (int e = w8_op_repack((hipStream_t)st, "fvhd_op_dec_gemm_w8", Wt, N, K, &a.W)) return e;
    a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = eps; a.wscale = scale; a.N = N; a.K = K; a.B = B; a.part = partial; a.cnt = counters;
    a.epi = epi; a.resid = resid; a.out = out; a.ldo = epi == FVHD_EPI_SWIGLU ? N / 2 : N;
    dec_split(a, splits);
    int e = fvhd_launch_dec_gemm((hipStream_t)st, &a);
    return e ? lhip("fvhd_op_dec_gemm_w8", (hipError_t)e) : 0;
}

int fvhd_op_dec_qkv_w8(fvhd_stream_t st, const void* x, int B, int K, const float* norm_w, float eps, const void* Wt, const float* scale, const float* bias,
                       void* q_out, const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache, void* v_cache, int capacity,
                       const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !scale || !bias || !q_out || !pos || !table || !k_cache || !v_cache || !length) return lfail("fvhd_op_dec_qkv_w8: NULL pointer");
    if (B < 1 || B > 64 || K < 128 || K % 128 || splits < 1 || head_dim < 16 || head_dim % 16 || n_heads < 1 || n_kv_heads < 1 || capacity < 1 ||
        table_positions < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_qkv_w8: needs 1 <= B <= 64, K % 128 == 0, head_dim % 16 == 0, splits >= 1 (and scratch when splits > 1)");
    DecGemmArgs a;
    a.N = (n_heads + 2 * n_kv_heads) * head_dim;
    if (int e = w8_op_repack((hipStream_t)st, "fvhd_op_dec_qkv_w8", Wt, a.N, K, &a.W)) return e;
    a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = eps; a.wscale = scale; a.K = K; a.B = B;
    a.part = partial; a.cnt = counters; a.epi = DEC_EPI_QKV; a.bias = bias; a.out = q_out; a.ldo = n_heads * head_dim; a.pos = pos; a.rope = table;
    a.P = table_positions; a.theta = rope_theta; a.nh = n_heads; a.nkv = n_kv_heads; a.hd = head_dim; a.kc = k_cache; a.vc = v_cache; a.cap = capacity;
    a.len = length;
    dec_split(a, splits);
    int e = fvhd_launch_dec_gemm((hipStream_t)st, &a);
    return e ? lhip("fvhd_op_dec_qkv_w8", (hipError_t)e) : 0;
}

int fvhd_op_dec_lm_argmax_w8(fvhd_stream_t st, const void* x, int B, const float* norm_w, float eps, const void* Wt, const float* scale, int V, int K,
                             float* logits, int64_t* ids_out, float* scratch_v, int* scratch_i)
{
    if (!x || !Wt || !scale || !ids_out || !scratch_v || !scratch_i) return lfail("fvhd_op_dec_lm_argmax_w8: NULL pointer");
    if (B < 1 || B > 64 || V < 16 || V % 16 || K < 128 || K % 128) return lfail("fvhd_op_dec_lm_argmax_w8: needs 1 <= B <= 64, V % 16 == 0, K % 128 == 0");
    DecGemmArgs a;
    if (int e = w8_op_repack((hipStream_t)st, "fvhd_op_dec_lm_argmax_w8", Wt, V, K, &a.W)) return e;
    a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = eps; a.wscale = scale; a.N = V; a.K = K; a.B = B; a.S = 1; a.cpw = K / 128; a.epi = DEC_EPI_ARGMAX;
    a.logits = logits; a.amax_v = scratch_v; a.amax_i = scratch_i;
    int e = fvhd_launch_dec_gemm((hipStream_t)st, &a);
    if (!e) e = fvhd_launch_dec_argmax_finish((hipStream_t)st, scratch_v, scratch_i, (V / 16 + 3) / 4, B, nullptr, ids_out, nullptr, nullptr, nullptr);
    return e ? lhip("fvhd_op_dec_lm_argmax_w8", (hipError_t)e) : 0;
}

// the sampler on its own: a process-wide workspace, allocated (and its counters zeroed) on first use - eager calls only
int fvhd_op_dec_sample(fvhd_stream_t st, const float* logits, int B, int V, float temperature, int top_k, float top_p, unsigned long long seed, int n,
                       const float* u_override, int64_t* ids, float* info)
{
    if (!logits || !ids) return lfail("fvhd_op_dec_sample: NULL pointer");
    if (B < 1 || B > 16 || V < 1) return lfail("fvhd_op_dec_sample: needs 1 <= B <= 16 and V >= 1");
    if (const char* e = sampling_error(temperature, top_k, top_p)) return lfail(std::string("fvhd_op_dec_sample: ") + e);
    static char* ws[64] = {};
    int dev = 0;
    hipError_t he = hipGetDevice(&dev);
    if (he != hipSuccess) return lhip("hipGetDevice", he);
    if (dev < 0 || dev >= 64) return lfail("fvhd_op_dec_sample: device index out of range");
    if (!ws[dev]) {
        const size_t bytes = fvhd_dec_sample_ws_bytes();
        if ((he = hipMalloc((void**)&ws[dev], bytes)) != hipSuccess) { ws[dev] = nullptr; return lhip("hipMalloc(sampler workspace)", he); }
        if ((he = hipMemset(ws[dev], 0, bytes)) != hipSuccess) return lhip("hipMemset(sampler workspace)", he);
    }
    DecSampleArgs a;
    a.logits = logits; a.B = B; a.V = V; a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.n_add = n;
    a.u_override = u_override; a.ids_out = ids; a.info = info;
    int e = fvhd_launch_dec_sample((hipStream_t)st, &a, ws[dev]);
    return e ? lhip("fvhd_op_dec_sample", (hipError_t)e) : 0;
}

}  // extern "C"
