"""TEST INFRASTRUCTURE ONLY - what the MXFP4 (4-bit weight) test files share: the planted rows of the recipe tests, random plain-order
codes / scales, the MXFP4 twin of `llm_testlib.models(..., quantised=True)` and the launch wrappers of the *_w4 single ops.  Importing it
needs no GPU."""
import torch

import llm_testlib as L
from ml_fastvlm_amd import _lib

W4 = "mxfp4"
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)                   # midpoints of the e2m1 grid, in units of the block scale
TIE_INDEX = (0, 2, 2, 4, 4, 6, 6)                                # the even index each lands on


def dequantised(w):
    """w -> bf16 values of its MXFP4 codes (exact in bf16)"""
    from ml_fastvlm_amd import dequantize_blocks_mxfp4, quantize_blocks_mxfp4
    return dequantize_blocks_mxfp4(*quantize_blocks_mxfp4(w))


def planted_rows(K):
    """[8, K] fp32 rows of bf16 values that exercise the recipe's corners, K % 32 == 0, K >= 64:
    0 zero row; 1 a zero block among random ones; 2 every tie (both signs) in a block whose amax is 6 (scale 1) and in one scaled by 2^-9;
    3 block amax with m just below, at and just above 1.5 (blocks 0, 1, 2 when K >= 96); 4 signed zeros and tiny negatives beside a large
    value; 5 the lower clamp (bf16 denormals and the smallest normals); 6 the upper clamp (values that saturate); 7 values over 36 binades"""
    g = torch.Generator().manual_seed(K)
    w = torch.zeros(8, K)
    w[1] = torch.randn(K, generator=g)
    w[1, 32:64] = 0
    t = torch.tensor(TIES)
    blk = torch.zeros(32)
    blk[0] = 6.0
    blk[1:8], blk[8:15] = t, -t
    blk[15], blk[16] = -6.0, 4.0
    w[2, :32] = blk
    w[2, 32:64] = blk * 2.0 ** -9
    for i, m in enumerate((1.4921875, 1.5, 1.5078125)):           # bf16 neighbours of 1.5
        if 32 * i + 32 <= K:
            w[3, 32 * i:32 * i + 32] = (0.01 * torch.randn(32, generator=g)).clamp(-0.04, 0.04)
            w[3, 32 * i + 5] = -m * 2.0 ** (i - 3)
    w[4, 0], w[4, 1], w[4, 2], w[4, 3], w[4, 4] = 3.0, -0.0, -1e-6, 1e-6, -0.7
    w[5, :32] = torch.tensor([2.0 ** -133, -(2.0 ** -130), 2.0 ** -126, -1.5 * 2.0 ** -126] * 8)
    w[5, 32:64] = torch.tensor([2.0 ** -124, -(2.0 ** -126), 3 * 2.0 ** -126, 0.0] * 8)
    w[6, :32] = torch.tensor([2.0 ** 127 * 1.75, -(2.0 ** 127) * 1.9921875, 2.0 ** 127, 2.0 ** 120] * 8)
    w[6, 32:64] = torch.tensor([2.0 ** 127 * 1.5, -(2.0 ** 125), 2.0 ** 126 * 1.25, 0.0] * 8)
    w[7] = torch.randn(K, generator=g) * torch.exp2(torch.randint(-18, 18, (K,), generator=g).float())
    exact = w[[2, 5, 6]].clone()
    w = w.to(torch.bfloat16).float()                              # (the random values, 1e-6 and 0.7 are rounded here)
    assert torch.equal(w[[2, 5, 6]], exact), "the tie and clamp rows are bf16 values as written"
    return w


def random_plain(N, K, g, device="cuda", e_lo=100, e_hi=150):
    """random codes u8 [N, K / 2] (every code, both zeros) and scale bytes u8 [N, K / 32] uniform in [e_lo, e_hi]: 2^-27 .. 2^23, 50
    binades, where bf16 products and fp32 sums of a decode GEMM stay finite"""
    codes = torch.randint(0, 256, (N, K // 2), device=device, generator=g, dtype=torch.uint8)
    scales = torch.randint(e_lo, e_hi + 1, (N, K // 32), device=device, generator=g, dtype=torch.uint8)
    return codes, scales


def models(name, seed=0, vocab=4096, layers=None):
    """(bf16 model holding MXFP4-dequantised matrices, fp32 oracle on the same values): `L.models(name)` with every 2-D decoder / lm_head weight (a tied model's table too) replaced by its dequantised value before the fp32
    copy is made"""
    from transformers import Qwen2ForCausalLM
    m16, _ = L.models(name, seed=seed, vocab=vocab, layers=layers)
    cfg = m16.config
    emb = m16.get_input_embeddings().weight
    with torch.no_grad():
        for p in m16.parameters():
            if p.dim() == 2 and (p is not emb or cfg.tie_word_embeddings):
                p.copy_(dequantised(p))
    ref = Qwen2ForCausalLM(cfg).eval().to("cuda")
    ref.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    return m16, ref


# ---- launches of the single ops ------------------------------------------------------------------------------------------------------
def dec_gemm_w4(lib, epi, x, nw, codes, scales, resid, splits):
    """one fvhd_op_dec_gemm_w4 launch into an `L.guarded` buffer -> out [B, width] (a copy); asserts the guard rows and the counters"""
    B, K = x.shape
    N = codes.shape[0]
    swiglu = epi == "swiglu"
    width = N // 2 if swiglu else N
    buf, out = L.guarded(B, width, "cuda")
    part, cnt = L.gemm_scratch(N, B, splits)
    L.check(lib.fvhd_op_dec_gemm_w4(L.stream(), _lib.EPI_SWIGLU if swiglu else _lib.EPI_RESID, L.ptr(x), B, L.ptr(nw), 1e-6, L.ptr(codes), L.ptr(scales), N, K,
                                    L.ptr(resid), L.ptr(out), L.ptr(part), L.ptr(cnt), splits), "dec_gemm_w4")
    torch.cuda.synchronize()
    assert L.guard_intact(buf, B), "rows >= B were written"
    assert cnt is None or int(cnt.abs().sum()) == 0, "counters not back at zero"
    return out.clone()


def dec_lm_argmax_w4(lib, x, nw, codes, scales, logits=True):
    B, H = x.shape
    V = codes.shape[0]
    lbuf = torch.full((B * V + 64,), float("nan"), device="cuda") if logits else None
    lg = lbuf[:B * V].view(B, V) if logits else None
    ids = torch.full((B + 4,), -7, device="cuda", dtype=torch.long)
    nblk = (V // 16 + 3) // 4
    sv = torch.empty(nblk * 16 * L.nb(B), device="cuda")
    si = torch.empty(nblk * 16 * L.nb(B), device="cuda", dtype=torch.int32)
    L.check(lib.fvhd_op_dec_lm_argmax_w4(L.stream(), L.ptr(x), B, L.ptr(nw), 1e-6, L.ptr(codes), L.ptr(scales), V, H, L.ptr(lg), L.ptr(ids), L.ptr(sv),
                                         L.ptr(si)), "lm_argmax_w4")
    torch.cuda.synchronize()
    assert bool((ids[B:] == -7).all())
    if logits:
        assert bool(torch.isnan(lbuf[B * V:]).all()), "the logits' guard tail was written"
    return lg, ids[:B].clone()
