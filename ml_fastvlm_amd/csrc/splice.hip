// Multimodal embedding splice: the data movement of LlavaMetaForCausalLM.prepare_inputs_labels_for_multimodal
// (llava/model/llava_arch.py:233-332) as ONE gather kernel.
//
// The reference walks the batch in Python: per sample it splits input_ids at the IMAGE_TOKEN_INDEX (-200) sentinels, embeds the
// text pieces, torch.cat's them with the image features, pads every sequence to the longest and builds attention mask, position
// ids and labels with per-sample slice assignments (a few dozen small launches and several host syncs per sample, all on the
// time-to-first-token path).  Here the host computes, with a handful of batched tensor ops (ml_fastvlm_amd/splice.py), where
// every kept input token STARTS in its output sequence; this kernel then produces every output row independently:
//   row (b, t):  binary search of t in the sample's start positions -> input token j;
//                text token  -> copy row ids[b, j] of the embedding table (llava_arch.py:257, 272);
//                image token -> copy row feat_row0[b, j] + (t - start) of the image features (llava_arch.py:279-283);
//                padding     -> zeros (llava_arch.py:306-322);   plus attention_mask / position_ids / labels of that row.
// One 256-thread workgroup copies 4 rows, 64 lanes x 16 B per step: HBM-bound, B x max_len x H x 2 bytes in and out.
#include "fvhd_common.h"
#include "launchers.h"

#define SPLICE_IGNORE (-100L)        /* IGNORE_INDEX, llava/constants.py:7 */

template <typename T>
__global__ __launch_bounds__(256) void splice_kernel(
    const long* __restrict__ ids, const int* __restrict__ start, const int* __restrict__ seqlen, const long* __restrict__ feat_row0,
    const long* __restrict__ labels_in, const T* __restrict__ table, const T* __restrict__ feats, T* __restrict__ out,
    unsigned char* __restrict__ mask_out, long* __restrict__ pos_out, long* __restrict__ labels_out,
    int B, int L, int H, int max_len, long vocab, long n_feat_rows, int left_pad)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)B * max_len) return;
    const int b = (int)(row / max_len), t = (int)(row - (long)b * max_len);
    const int len = seqlen[b];                       // tokens of this sample after the splice (already truncated)
    const int shift = left_pad ? max_len - len : 0;  // tokenizer_padding_side == "left" (llava_arch.py:306-314)
    const int u = t - shift;                         // position inside the spliced sequence
    T* dst = out + row * H;
    const bool valid = u >= 0 && u < len;
    const T* src = nullptr;
    long lab = SPLICE_IGNORE;
    if (valid) {
        // last input position j with start[b, j] <= u  (start is non-decreasing along j; dropped tokens repeat their successor's start
        // and have length 0, so the search lands on the token that owns u)
        const int* st = start + (long)b * L;
        int lo = 0, hi = L - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (st[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const long id = ids[(long)b * L + lo];
        const long f0 = feat_row0[(long)b * L + lo];
        if (f0 >= 0) {                               // image token: feature row f0 + offset inside the image
            const long fr = f0 + (u - st[lo]);
            src = fr < n_feat_rows ? feats + fr * H : nullptr;
        } else {
            src = (id >= 0 && id < vocab) ? table + id * H : nullptr;
            if (labels_in) lab = labels_in[(long)b * L + lo];
        }
    }
    constexpr int VPL = 16 / sizeof(T);              // elements per 16-B lane access
    for (int c = lane * VPL; c < H; c += 64 * VPL) {
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (src) v = *(const u32x4*)(src + c);
        *(u32x4*)(dst + c) = v;
    }
    if (lane == 0) {
        if (mask_out) mask_out[row] = valid ? 1 : 0;
        if (pos_out) pos_out[row] = valid ? (long)u : 0L;     // arange(cur_len) in the valid span, 0 in the padding (llava_arch.py:300, 313, 322)
        if (labels_out) labels_out[row] = lab;
    }
}

// ids [B, L] int64 (input ids with the -200 sentinels; dropped positions may hold anything), start [B, L] int32 (see the kernel),
// seqlen [B] int32, feat_row0 [B, L] int64 (-1 for text), labels_in [B, L] int64 or null, table [vocab, H], feats [n_feat_rows, H],
// out [B, max_len, H]; mask_out u8 / pos_out int64 / labels_out int64 [B, max_len] or null.  dtype: FVHD_F32 / F16 / BF16; H % 8 == 0
// (16-B vectors for 2-byte types; H % 4 for fp32).
extern "C" int fvhd_launch_splice(hipStream_t st, const long* ids, const int* start, const int* seqlen, const long* feat_row0,
                                  const long* labels_in, const void* table, const void* feats, void* out, unsigned char* mask_out,
                                  long* pos_out, long* labels_out, int B, int L, int H, int max_len, long vocab, long n_feat_rows,
                                  int left_pad, int dtype)
{
    if (B <= 0 || L <= 0 || H <= 0 || max_len <= 0) return (int)hipErrorInvalidValue;
    if (dtype == FVHD_F32 ? (H % 4) : (H % 8)) return (int)hipErrorInvalidValue;
    const long rows = (long)B * max_len;
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    if (dtype == FVHD_F32)
        hipLaunchKernelGGL(splice_kernel<float>, grid, block, 0, st, ids, start, seqlen, feat_row0, labels_in, (const float*)table,
                           (const float*)feats, (float*)out, mask_out, pos_out, labels_out, B, L, H, max_len, vocab, n_feat_rows, left_pad);
    else
        hipLaunchKernelGGL(splice_kernel<unsigned short>, grid, block, 0, st, ids, start, seqlen, feat_row0, labels_in,
                           (const unsigned short*)table, (const unsigned short*)feats, (unsigned short*)out, mask_out, pos_out, labels_out,
                           B, L, H, max_len, vocab, n_feat_rows, left_pad);
    return (int)hipGetLastError();
}
