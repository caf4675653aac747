// C ABI of the Qwen2 language model (include/fvhd.h "LLM prefill"): the context and its packed weights - creation, the weight format,
// the layout of the matrices in `wdev`, and the tensors of the state dict arriving from host or device memory.
#include <stdlib.h>
#include <string.h>

#include "llm_ctx.h"

namespace {

float load_as_float(const void* p, int dtype, size_t i)
{
    if (dtype == FVHD_F32) return ((const float*)p)[i];
    if (dtype == FVHD_BF16) { uint32_t u = (uint32_t)((const uint16_t*)p)[i] << 16; float f; memcpy(&f, &u, 4); return f; }
    _Float16 h;                             // IEEE half to float is exact (a signalling-NaN half may come out as a quiet NaN)
    memcpy(&h, (const uint16_t*)p + i, 2);
    return (float)h;
}

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
    const bool q8 = c->wfmt == FVHD_W_E4M3, q4 = c->wfmt == FVHD_W_MXFP4;
    // bytes of N * K matrix elements, and of their scales: e4m3 one fp32 per row, MXFP4 one byte per 32 elements (K % 128 == 0)
    auto mb = [&](size_t N, size_t K) { return q4 ? N * K / 2 : q8 ? N * K : N * K * 2; };
    auto sb = [&](size_t N, size_t K) { return q4 ? N * K / 32 : N * 4; };
    Arena a;
    c->lo.assign(c->L, LayerOff{});
    for (int l = 0; l < c->L; ++l) {
        LayerOff& o = c->lo[l];
        o.ln1 = a.take(H * 4);
        o.w[FVHD_MAT_QKV] = a.take(mb(qkvw, H));
        o.bqkv = a.take(qkvw * 4);
        o.w[FVHD_MAT_O] = a.take(mb(H, ao));
        o.ln2 = a.take(H * 4);
        o.w[FVHD_MAT_GATE_UP] = a.take(mb(2 * I, H));
        o.w[FVHD_MAT_DOWN] = a.take(mb(H, I));
        if (q8 || q4) {
            o.s[FVHD_MAT_QKV] = a.take(sb(qkvw, H)); o.s[FVHD_MAT_O] = a.take(sb(H, ao));
            o.s[FVHD_MAT_GATE_UP] = a.take(sb(2 * I, H)); o.s[FVHD_MAT_DOWN] = a.take(sb(H, I));
        }
    }
    c->norm_off = a.take(H * 4);
    c->lm_off = a.take(mb(V, H));
    c->lm_soff = q8 || q4 ? a.take(sb(V, H)) : 0;
    c->wbytes = a.off;
}

// where a tensor of the state dict goes: cols == 0: `rows` floats at base + 4 eoff; else a [rows][cols] matrix whose element (0, 0) is
// element eoff of the packed matrix at `base`, rows `pitch` elements apart (gate / up: interleaved rows), and - e4m3 - whose row scales
// start at float seoff of `sbase`, one every `sstride` floats (MXFP4: the scale bytes of row r are the cols / 32 bytes at
// sbase + (seoff + r * sstride) * cols / 32, the codes of element (0, 0) at base + eoff / 2)
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
    case 1: s.base = o.w[FVHD_MAT_QKV]; s.rows = nh * hd; s.cols = H; s.pitch = H; s.sbase = o.s[FVHD_MAT_QKV]; break;
    case 2: s.base = o.bqkv; s.rows = nh * hd; break;
    case 3: s.base = o.w[FVHD_MAT_QKV]; s.eoff = nh * hd * H; s.rows = nkv * hd; s.cols = H; s.pitch = H; s.sbase = o.s[FVHD_MAT_QKV]; s.seoff = nh * hd; break;
    case 4: s.base = o.bqkv; s.eoff = nh * hd; s.rows = nkv * hd; break;
    case 5: s.base = o.w[FVHD_MAT_QKV]; s.eoff = (nh + nkv) * hd * H; s.rows = nkv * hd; s.cols = H; s.pitch = H; s.sbase = o.s[FVHD_MAT_QKV]; s.seoff = (nh + nkv) * hd; break;
    case 6: s.base = o.bqkv; s.eoff = (nh + nkv) * hd; s.rows = nkv * hd; break;
    case 7: s.base = o.w[FVHD_MAT_O]; s.rows = H; s.cols = nh * hd; s.pitch = nh * hd; s.sbase = o.s[FVHD_MAT_O]; break;
    case 8: s.base = o.ln2; s.rows = H; break;
    // gate / up rows interleaved (row 2j = gate_j, row 2j + 1 = up_j): the SwiGLU epilogue of the GEMM pairs adjacent columns
    case 9: s.base = o.w[FVHD_MAT_GATE_UP]; s.rows = I; s.cols = H; s.pitch = 2 * H; s.sbase = o.s[FVHD_MAT_GATE_UP]; s.sstride = 2; break;
    case 10: s.base = o.w[FVHD_MAT_GATE_UP]; s.eoff = H; s.rows = I; s.cols = H; s.pitch = 2 * H; s.sbase = o.s[FVHD_MAT_GATE_UP]; s.seoff = 1; s.sstride = 2; break;
    case 11: s.base = o.w[FVHD_MAT_DOWN]; s.rows = H; s.cols = I; s.pitch = I; s.sbase = o.s[FVHD_MAT_DOWN]; break;
    }
    return s;
}

// e4m3: bf16 rows [rows][cols] on the device -> codes + scales at the slot (rows are whole, so every source tensor quantises on its own)
int quantize_into(fvhd_llm* c, const Slot& s, const void* dev_bf16, hipStream_t st)
{
    return lret("quantise to e4m3", fvhd_launch_quantize_e4m3(st, dev_bf16, (int)s.rows, (int)s.cols, c->wdev + s.base + s.eoff, (long)s.pitch,
                                                              (float*)(c->wdev + s.sbase) + s.seoff, s.sstride, 1));
}

// MXFP4: the same rows -> codes + block scales at the slot
int quantize_into_w4(fvhd_llm* c, const Slot& s, const void* dev_bf16, hipStream_t st)
{
    const size_t spr = s.cols / 32;       // scale bytes per row
    return lret("quantise to MXFP4", fvhd_launch_quantize_mxfp4(st, dev_bf16, (int)s.rows, (int)s.cols, c->wdev + s.base + s.eoff / 2, (long)(s.pitch / 2),
                                                                c->wdev + s.sbase + s.seoff * spr, (long)(s.sstride * spr), 1));
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
        for (size_t i = 0; i < rows * cols; ++i) tmp[i] = f32_to_bf16_rne(load_as_float(host, dtype, i));
    hipError_t e = hipMemcpy2D(dst, pitch_elems * 2, tmp.data(), cols * 2, cols * 2, rows, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : lhip("hipMemcpy2D(llm weights)", e);
}

// e4m3 / MXFP4: the same host rows through a bf16 staging buffer on the device and the quantise kernel
int upload_matrix_q(fvhd_llm* c, const void* host, int dtype, const Slot& s)
{
    char* stage = nullptr;
    hipError_t e = hipMalloc((void**)&stage, s.rows * s.cols * 2);
    if (e != hipSuccess) return lhip("hipMalloc(quantise staging)", e);
    int r = upload_matrix(host, dtype, s.rows, s.cols, stage, s.cols);
    if (!r) r = c->wfmt == FVHD_W_MXFP4 ? quantize_into_w4(c, s, stage, nullptr) : quantize_into(c, s, stage, nullptr);
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

}  // namespace

Mat mat_of(const fvhd_llm* c, int layer, int matrix)
{
    const long N[5] = {c->qkvw, c->H, 2 * (long)c->I, c->H, c->V};
    const int K[5] = {c->H, c->nh * c->hd, c->H, c->I, c->H};
    if (matrix == FVHD_MAT_LM_HEAD) return {c->lm_off, c->lm_soff, N[matrix], K[matrix]};
    return {c->lo[layer].w[matrix], c->lo[layer].s[matrix], N[matrix], K[matrix]};
}

int first_missing_tensor(const fvhd_llm* c)
{
    for (size_t i = 0; i < c->got.size(); ++i)
        if (!c->got[i]) return (int)i;
    return -1;
}

// every copy fvhd_llm_set_tensor_device has enqueued so far has completed (host wait); the caller holds a DeviceGuard
int wait_for_loads(fvhd_llm* c)
{
    if (!c->load_pending) return 0;
    const hipError_t e = hipEventSynchronize(c->load_ev);
    if (e != hipSuccess) return lhip("hipEventSynchronize(llm weights)", e);
    c->load_pending = false;
    return 0;
}

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
    DeviceGuard g(device);
    if (g.err != hipSuccess) { delete c; return lhip("hipSetDevice", g.err); }
    hipError_t e = hipMalloc((void**)&c->wdev, c->wbytes);
    if (e != hipSuccess) { delete c; return lhip("hipMalloc(llm weights)", e); }
    *out = c;
    return 0;
}

void fvhd_llm_destroy(fvhd_llm* c)
{
    if (!c) return;
    DeviceGuard g(c->device);
    (void)hipDeviceSynchronize();
    if (c->wdev) (void)hipFree(c->wdev);
    if (c->wscratch) (void)hipFree(c->wscratch);
    if (c->ws) (void)hipFree(c->ws);
    for (char* p : c->retired) (void)hipFree(p);
    if (c->proc_lists) (void)hipFree(c->proc_lists);
    if (c->load_ev) (void)hipEventDestroy(c->load_ev);
    if (c->emb) (void)hipFree(c->emb);
    if (c->dc) (void)hipFree(c->dc);
    if (c->beam) (void)hipFree(c->beam);
    if (c->beam_sample) (void)hipFree(c->beam_sample);
    if (c->beam_proc) (void)hipFree(c->beam_proc);
    if (c->spec) (void)hipFree(c->spec);
    if (c->spx) (void)hipFree(c->spx);
    if (c->score_ws) (void)hipFree(c->score_ws);
    if (c->lp_ws) (void)hipFree(c->lp_ws);
    if (c->con_tab) (void)hipFree(c->con_tab);
    if (c->con_state) (void)hipFree(c->con_state);
    if (c->guid_ws) (void)hipFree(c->guid_ws);
    if (c->pre_kv) (void)hipFree(c->pre_kv);
    if (c->status_host) (void)hipHostFree(c->status_host);
    delete c;
}

int fvhd_llm_set_weight_format(fvhd_llm* c, int format)
{
    if (!c) return lfail("fvhd_llm_set_weight_format: ctx is NULL");
    if (format != FVHD_W_BF16 && format != FVHD_W_E4M3 && format != FVHD_W_MXFP4)
        return lfail("fvhd_llm_set_weight_format: format must be FVHD_W_BF16, FVHD_W_E4M3 or FVHD_W_MXFP4");
    if (c->any_set)
        return lfail("fvhd_llm_set_weight_format: a tensor was already set - choose the format right after fvhd_llm_create, before the first "
                     "fvhd_llm_set_tensor / fvhd_llm_set_tensor_device (the matrices are quantised as they arrive)");
    if (format == c->wfmt) return 0;
    if (format == FVHD_W_E4M3 && (c->H % 128 || (c->nh * c->hd) % 128 || c->I % 128))
        return lfail("fvhd_llm_set_weight_format: FVHD_W_E4M3 needs hidden, n_heads * head_dim and intermediate to be multiples of 128");
    if (format == FVHD_W_MXFP4 && (c->H % 128 || (c->nh * c->hd) % 128 || c->I % 128))
        return lfail("fvhd_llm_set_weight_format: FVHD_W_MXFP4 needs hidden, n_heads * head_dim and intermediate to be multiples of 128");
    LLM_ON_DEVICE(c);
    if (c->wdev) (void)hipFree(c->wdev);
    if (c->wscratch) (void)hipFree(c->wscratch);
    c->wdev = c->wscratch = nullptr;
    c->wscratch_bytes = 0;
    c->wfmt = format;
    weight_layout(c);
    hipError_t e = hipMalloc((void**)&c->wdev, c->wbytes);
    if (e != hipSuccess) return lhip("hipMalloc(llm weights)", e);
    if (format != FVHD_W_BF16) {
        for (int m = FVHD_MAT_QKV; m <= FVHD_MAT_LM_HEAD; ++m) {          // the largest matrix as bf16 (every layer has the same sizes)
            const Mat d = mat_of(c, 0, m);
            c->wscratch_bytes = std::max(c->wscratch_bytes, (size_t)d.N * d.K * 2);
        }
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
        LLM_ON_DEVICE(c);
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
    LLM_ON_DEVICE(c);
    if (!ok) return lfail(std::string("fvhd_llm_set_tensor: bad shape for ") + key);
    int e = 0;
    if (vec) e = upload_vector_f32(host_data, dtype, sl.rows, c->wdev + sl.base + sl.eoff * 4);
    else if (c->wfmt != FVHD_W_BF16) e = upload_matrix_q(c, host_data, dtype, sl);
    else e = upload_matrix(host_data, dtype, sl.rows, sl.cols, c->wdev + sl.base + sl.eoff * 2, sl.pitch);
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
        LLM_ON_DEVICE(c);
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
    LLM_ON_DEVICE(c);
    hipError_t e = hipSuccess;
    if (vec) e = hipMemcpyAsync(c->wdev + sl.base + sl.eoff * 4, dev_data, rows * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    else if (c->wfmt == FVHD_W_E4M3) {                          // quantised on `stream` straight from the caller's tensor
        if (int qe = quantize_into(c, sl, dev_data, (hipStream_t)stream)) return qe;
    } else if (c->wfmt == FVHD_W_MXFP4) {
        if (int qe = quantize_into_w4(c, sl, dev_data, (hipStream_t)stream)) return qe;
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

int fvhd_llm_finalize(fvhd_llm* c)
{
    if (!c) return lfail("fvhd_llm_finalize: ctx is NULL");
    if (const int i = first_missing_tensor(c); i >= 0)
        return lfail("fvhd_llm_finalize: missing tensor (layer " + std::to_string(i / 12) + ", slot " + std::to_string(i % 12) +
                     "; slots: ln1 q.w q.b k.w k.b v.w v.b o.w ln2 gate up down | norm lm_head)");
    LLM_ON_DEVICE(c);
    return wait_for_loads(c);               // the device-to-device packing is complete when this returns (include/fvhd.h "stream contract")
}

// one packed matrix of an e4m3 context in plain [N, K] order (the packing test): codes u8 [N][K], scales fp32 [N], device pointers
int fvhd_llm_debug_packed_e4m3(fvhd_llm* c, int layer, int matrix, void* codes_out, float* scale_out, fvhd_stream_t stream)
{
    if (!c || !codes_out || !scale_out) return lfail("fvhd_llm_debug_packed_e4m3: NULL argument");
    if (c->wfmt == FVHD_W_MXFP4) return lfail("fvhd_llm_debug_packed_e4m3: the context holds MXFP4 weights, not e4m3 (fvhd_llm_debug_packed_mxfp4)");
    if (c->wfmt != FVHD_W_E4M3) return lfail("fvhd_llm_debug_packed_e4m3: the context holds bf16 weights (fvhd_llm_set_weight_format)");
    if (matrix < FVHD_MAT_QKV || matrix > FVHD_MAT_LM_HEAD || (matrix != FVHD_MAT_LM_HEAD && (layer < 0 || layer >= c->L)))
        return lfail("fvhd_llm_debug_packed_e4m3: matrix must be FVHD_MAT_QKV .. FVHD_MAT_LM_HEAD and layer in [0, n_layers)");
    const Mat m = mat_of(c, layer, matrix);
    LLM_ON_DEVICE(c);
    if (int e = wait_for_loads(c)) return e;
    LCHECK(fvhd_launch_w8_unpack((hipStream_t)stream, c->wdev + m.off, nullptr, codes_out, m.N, m.K, 1), "fvhd_llm_debug_packed_e4m3");
    const hipError_t he = hipMemcpyAsync(scale_out, c->wdev + m.soff, (size_t)m.N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return he == hipSuccess ? 0 : lhip("hipMemcpyAsync", he);
}

// one packed matrix of an MXFP4 context in plain [N, K] order: codes u8 [N][K / 2], block scales u8 [N][K / 32], device pointers
int fvhd_llm_debug_packed_mxfp4(fvhd_llm* c, int layer, int matrix, void* codes_out, void* scales_out, fvhd_stream_t stream)
{
    if (!c || !codes_out || !scales_out) return lfail("fvhd_llm_debug_packed_mxfp4: NULL argument");
    if (c->wfmt != FVHD_W_MXFP4) return lfail("fvhd_llm_debug_packed_mxfp4: the context does not hold MXFP4 weights (fvhd_llm_set_weight_format)");
    if (matrix < FVHD_MAT_QKV || matrix > FVHD_MAT_LM_HEAD || (matrix != FVHD_MAT_LM_HEAD && (layer < 0 || layer >= c->L)))
        return lfail("fvhd_llm_debug_packed_mxfp4: matrix must be FVHD_MAT_QKV .. FVHD_MAT_LM_HEAD and layer in [0, n_layers)");
    const Mat m = mat_of(c, layer, matrix);
    LLM_ON_DEVICE(c);
    if (int e = wait_for_loads(c)) return e;
    LCHECK(fvhd_launch_w4_unpack((hipStream_t)stream, c->wdev + m.off, nullptr, codes_out, m.N, m.K, 1), "fvhd_llm_debug_packed_mxfp4");
    const hipError_t he = hipMemcpyAsync(scales_out, c->wdev + m.soff, (size_t)m.N * (m.K / 32), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return he == hipSuccess ? 0 : lhip("hipMemcpyAsync", he);
}

}  // extern "C"
