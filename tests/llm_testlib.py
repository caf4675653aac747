"""TEST INFRASTRUCTURE ONLY - the helpers the Qwen2 test files share, each defined once: C-ABI plumbing, the comparison contracts,
sentinel guards, the inputs and launch wrappers of the decode ops, the automaton, prompts and op wrappers of the step's logits edits, and
the small models with their fp32 oracles.  Imported as
decode_reference / prefill_reference are (after the tests directory is put on sys.path; a file that had its own copy of a helper binds
the shared one to the name it used, `from llm_testlib import ptr as _p`).  Importing it needs
no GPU: nothing here touches torch.cuda before a function is called, and `transformers` is imported by the functions that use it.

PINNING: tests/test_llm_testlib.py checks the per-row bound, both guard forms, `row_scales` and `padded_mask` on the CPU."""
import math

import pytest
import torch

from ml_fastvlm_amd import _lib

DEV = "cuda:0"                 # the device of compare_prefill

# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
ptr = _lib.ptr                 # tensor or None -> c_void_p
check = _lib.check


def stream(device=None):
    """the current stream of `device` (default: the current device) -> c_void_p"""
    return _lib.stream_ptr(device)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- comparison ------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def metrics(got, want):
    """-> (rel-L2, cosine, max |err| / max |want|)"""
    got, want = got.double().cpu().flatten(), want.double().cpu().flatten()
    rel = ((got - want).norm() / want.norm()).item()
    cos = torch.nn.functional.cosine_similarity(got, want, dim=0).item()
    mx = ((got - want).abs().max() / want.abs().max()).item()
    return rel, cos, mx


def violations(got, want, rtol, atol_rms, rows=None):
    """-> (elements outside |err| <= rtol |want| + atol_rms rms(want row), the largest err / bound): the project's accuracy contract for
    single ops, the rms PER ROW (rows of scales 0.05 .. 20 sit side by side in the tests, a pooled rms would hide the small ones).  A
    row is the LAST dimension (one (b, t, head) vector of hd values, one row of rmsnorm / rope); rows: bool mask over the leading
    dimensions of the rows to compare"""
    assert got.shape == want.shape, (got.shape, want.shape)
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(got).all()), "non-finite output"
    if rows is not None:
        got, want = got[rows], want[rows]
    if want.numel() == 0:
        return 0, 0.0
    rms = want.pow(2).mean(-1, keepdim=True).sqrt()
    err, bound = (got - want).abs(), rtol * want.abs() + atol_rms * rms
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return int((err > bound).sum()), float(ratio.max())


def close(got, want, what, rtol=1e-2, atol_rms=1e-2, rows=None):
    bad, worst = violations(got, want, rtol, atol_rms, rows)
    assert bad == 0, f"{what}: {bad} of {want.numel()} elements out of tolerance, worst err / bound {worst:.3g}"
    return worst


def close_by_batch_row(got, want, what, rtol=1e-2, atol_rms=1e-2):
    """close() with a row = everything but dim 0: one sequence of a decode step"""
    return close(got.double().reshape(got.shape[0], -1), want.double().reshape(want.shape[0], -1), what, rtol, atol_rms)


def close_pooled(got, want, what="", rtol=1e-2, atol_rms=1e-2):
    """|err| <= rtol |want| + atol_rms rms(want), ONE rms over the whole tensor: the budget of the tower's and the prefill's first op
    tests, looser per row than close() wherever the rows differ in scale"""
    got, want = got.float().cpu(), want.float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    rms = want.pow(2).mean().sqrt().item()
    err = (got - want).abs()
    bound = rtol * want.abs() + atol_rms * rms
    bad = (err > bound).sum().item()
    assert bad == 0, f"{what}: {bad}/{err.numel()} elements out of tolerance, max err {err.max():.4g}, rms {rms:.4g}"


def bf(t):
    """rounded to bf16, back in fp32"""
    return t.to(torch.bfloat16).float()


# ---- sentinel guards -------------------------------------------------------------------------------------------------------------------
SENT = 0x7B3D                  # bf16 bit pattern of the guard fill (1.23e36): no kernel output takes it by chance


def guarded(rows, width, device, guard_rows=64):
    """a [rows + guard_rows, width] bf16 buffer filled with the sentinel -> (the whole buffer as int16 [rows + guard_rows, width],
    the bf16 view of its first `rows` rows)"""
    buf = torch.full((rows + guard_rows, width), SENT, device=device, dtype=torch.int16)
    return buf, buf.view(torch.bfloat16)[:rows]


def guarded_rows(width, B, device="cuda"):
    """the flat form of the decode ops: max(16, B + 2) rows of `width` + 64 guard elements, sentinel-filled -> (the buffer as int16,
    the [B, width] bf16 view of its head)"""
    buf = torch.full((max(16, B + 2) * width + 64,), SENT, device=device, dtype=torch.int16)
    return buf, buf.view(torch.bfloat16)[:B * width].view(B, width)


def guard_intact(buf, used):
    """used: rows of a guarded() buffer, elements of a guarded_rows() one"""
    return bool((buf[used:] == SENT).all())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.int16) == b.contiguous().view(torch.int16)).all())


# ---- decode ops: inputs ----------------------------------------------------------------------------------------------------------------
# the ragged last workgroup, N / 16 % 4 = 1 (N = 16, 80, 912, 4880), 2 (32, 928, 4896) and 3 (48, 4912), beside the model widths
# (remainder 0); K in {128, 256, 896, 4864} beside the model depths
GEMM_SHAPES = [(16, 128), (32, 128), (48, 256), (80, 896), (912, 4864), (928, 896), (4880, 896), (4896, 256), (4912, 4864), (896, 896), (896, 4864), (9728, 896), (1536, 8960), (17920, 1536),
               (3584, 18944), (37888, 3584)]


def row_scales(B, g, device="cuda"):
    """distinct factors spanning 0.05 .. 20, shuffled, a fresh permutation for every block of 16 rows; one row: 20 (after the draw)"""
    base = torch.logspace(math.log10(0.05), math.log10(20.0), 16, device=device, dtype=torch.float32)
    s = torch.cat([base[torch.randperm(16, device=device, generator=g)] for _ in range((B + 15) // 16)])
    return s[:B] if B > 1 else s.new_tensor([20.0])


def padded_mask(B, cap, length, side, step=None, wrap=None, device="cuda"):
    """row b: step * (b + 1) padded keys (capped below the length; wrap = 13: step * (b % 13 + 1), so that a wide batch keeps valid
    keys), step 150 for a long cache (whole 64-key blocks and whole 128-key slices masked, from row 0 on) and a fifth of a short one"""
    if step is None:
        step = 150 if length > 600 else max(length // 5, 1)
    mask = torch.zeros(B, cap, device=device, dtype=torch.uint8)
    for b in range(B):
        npad = min(step * ((b if wrap is None else b % wrap) + 1), length - 1)
        if side == "left":
            mask[b, npad:length] = 1
        else:
            mask[b, :length - npad] = 1
    return mask


def nb(B):
    """batch tiles of 16 rows"""
    return (B + 15) // 16


def blocks(B):
    return [(i, min(i + 16, B)) for i in range(0, B, 16)]


def plan_splits(N, K):
    """the step's own choice (dec_plan in csrc/llm_step.hip): K split until the grid holds about two workgroups per CU, at most 16"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    ncol, KC = (N // 16 + 3) // 4, K // 128
    S = max(1, min((2 * ncu + ncol - 1) // ncol, KC, 16))
    cpw = (KC + S - 1) // S
    return (KC + cpw - 1) // cpw


def lowest_argmax(lg):
    V = lg.shape[1]
    idx = torch.arange(V, device=lg.device)[None].expand_as(lg)
    return torch.where(lg == lg.max(-1, keepdim=True).values, idx, torch.full_like(idx, V)).min(-1).values


# ---- decode ops: launches --------------------------------------------------------------------------------------------------------------
def gemm_scratch(N, B, splits):
    """(fp32 partial sums, zeroed counters) of a split weight-streaming GEMM; splits == 1: NULL, NULL"""
    part = torch.empty(splits * N * 16 * nb(B), device="cuda") if splits > 1 else None
    cnt = torch.zeros((N // 16 + 3) // 4, device="cuda", dtype=torch.int32) if splits > 1 else None
    return part, cnt


def dec_gemm(lib, epi, x, nw, W, resid, splits, alias=False):
    """one fvhd_op_dec_gemm launch into a guarded buffer -> out [B, width] (a copy).  Asserts that rows >= B and the guard tail keep the
    sentinel and that the counters are back at zero.  alias: the model's form, resid IS out"""
    B, K = x.shape
    N = W.shape[0]
    swiglu = epi == "swiglu"
    width = N // 2 if swiglu else N
    buf, out = guarded_rows(width, B)
    part, cnt = gemm_scratch(N, B, splits)
    if alias:
        out.copy_(resid)
        resid = out
    check(lib.fvhd_op_dec_gemm(stream(), _lib.EPI_SWIGLU if swiglu else _lib.EPI_RESID, ptr(x), B, ptr(nw), 1e-6, ptr(W), N, K, ptr(resid), ptr(out),
                               ptr(part), ptr(cnt), splits), "dec_gemm")
    torch.cuda.synchronize()
    assert guard_intact(buf, B * width), "rows >= B or the guard tail were written"
    assert cnt is None or int(cnt.abs().sum()) == 0, "counters not back at zero"
    return out.clone()


def dec_attention(lib, q, kc, vc, mask, length, splits):
    B, nkv, cap, hd = kc.shape
    nh = q.shape[1] // hd
    buf, out = guarded_rows(nh * hd, B)
    ln = torch.tensor([length], device="cuda", dtype=torch.int32)
    part = torch.empty(B * nh * splits * (hd + 2), device="cuda") if splits > 1 else None
    cnt = torch.zeros(B * nh, device="cuda", dtype=torch.int32) if splits > 1 else None
    check(lib.fvhd_op_dec_attention(stream(), ptr(q), ptr(kc), ptr(vc), ptr(mask), ptr(out), B, nh, nkv, hd, cap, ptr(ln), ptr(part), ptr(cnt), splits),
          "dec_attention")
    torch.cuda.synchronize()
    assert guard_intact(buf, B * nh * hd), "rows >= B or the guard tail were written"
    assert cnt is None or int(cnt.abs().sum()) == 0, "counters not back at zero"
    return out.clone()


def dec_lm_argmax(lib, x, nw, W, logits=True):
    """-> (fp32 logits [B, V] or None, ids [B]); the logits sit before a NaN guard tail, the ids before four guard entries"""
    B, H = x.shape
    V = W.shape[0]
    lbuf = torch.full((B * V + 64,), float("nan"), device="cuda") if logits else None
    lg = lbuf[:B * V].view(B, V) if logits else None
    ids = torch.full((B + 4,), -7, device="cuda", dtype=torch.long)
    nblk = (V // 16 + 3) // 4
    sv = torch.empty(nblk * 16 * nb(B), device="cuda")
    si = torch.empty(nblk * 16 * nb(B), device="cuda", dtype=torch.int32)
    check(lib.fvhd_op_dec_lm_argmax(stream(), ptr(x), B, ptr(nw), 1e-6, ptr(W), V, H, ptr(lg), ptr(ids), ptr(sv), ptr(si)), "lm_argmax")
    torch.cuda.synchronize()
    assert bool((ids[B:] == -7).all())
    if logits:
        assert bool(torch.isnan(lbuf[B * V:]).all()), "the logits' guard tail was written"
    return lg, ids[:B].clone()


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
def sample(lib, logits, T, k, p, seed=0, n=0, u=None):
    """one fvhd_op_dec_sample launch -> (ids [B], info [B, 4]: theta, kept count, Z, u)"""
    B, V = logits.shape
    ids = torch.full((B,), -1, device="cuda", dtype=torch.long)
    info = torch.zeros(B, 4, device="cuda")
    check(lib.fvhd_op_dec_sample(stream(), ptr(logits), B, V, float(T), int(k), float(p), int(seed), int(n), ptr(u), ptr(ids), ptr(info)),
          "fvhd_op_dec_sample")
    torch.cuda.synchronize()
    return ids, info


def oracle_scores(logits, T, k, p):
    """transformers' warpers, in _get_logits_processor's order -> processed scores (-inf = removed), on the host: there `scores / T` is
    the IEEE division (torch on the GPU divides by a host scalar as a multiply by its reciprocal, which can differ by one ulp)"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = logits.detach().float().cpu().clone()
    if T != 1.0:
        s = TemperatureLogitsWarper(T)(None, s)
    if k > 0:
        s = TopKLogitsWarper(k)(None, s)
    if p < 1.0:
        s = TopPLogitsWarper(p)(None, s)
    return s


# ---- the step's logits edits: what the constraint, guidance and step-chain tests share -------------------------------------------------
def bits(t):
    """fp32 -> its int32 bit patterns (a bit-for-bit comparison tells -0 from +0 and one NaN from another)"""
    return t.contiguous().view(torch.int32)


AUTOMATON_SIZES = (3, 5, 40, 2000, 7, 1)
AUTOMATON_WIDE = (300, 500, 400, 2000, 70, 100)      # under the processors: no state whose every edge an n-gram ban could take (such a row is undefined)


def make_automaton(seed=0, vocab=4096, sizes=AUTOMATON_SIZES):
    """6 states; state 0: three tokens that all lead back to it; state 4 has an edge to FREE; the others wander among 1 .. 5"""
    from ml_fastvlm_amd.constraints import FREE, TokenAutomaton
    g = torch.Generator().manual_seed(seed)
    offsets, tokens, targets = [0], [], []
    for s, k in enumerate(sizes):
        ids = torch.randperm(vocab, generator=g)[:k].sort().values.tolist()
        tokens += ids
        tgt = [0] * k if s == 0 else (1 + torch.randint(0, 5, (k,), generator=g)).tolist()
        if s == 4:
            tgt[0] = FREE
        targets += tgt
        offsets.append(len(tokens))
    return TokenAutomaton(offsets, tokens, targets, vocab)


def automaton_starts(B, n_states):
    """rows in different start states, row 1 unconstrained"""
    from ml_fastvlm_amd.constraints import FREE
    return [FREE if b == 1 else (b * 5 + 1) % n_states for b in range(B)]


def op_logprobs(lib, x, ids, n):
    """one fvhd_op_dec_logprobs launch on x fp32 [B, W] and ids int64 [B] -> (token log-probabilities [B], top ids [B, n], theirs [B, n])"""
    B, W = x.shape
    nbytes = lib.fvhd_dec_logprobs_scratch_bytes(B, W, n)
    scratch = torch.zeros(nbytes, device="cuda", dtype=torch.uint8)
    tok = torch.zeros(B, device="cuda")
    top = torch.zeros(B, n, device="cuda", dtype=torch.long)
    top_lp = torch.zeros(B, n, device="cuda")
    check(lib.fvhd_op_dec_logprobs(stream(), ptr(x), ptr(ids), B, W, n, ptr(tok), ptr(top), ptr(top_lp), ptr(scratch), nbytes), "fvhd_op_dec_logprobs")
    torch.cuda.synchronize()
    return tok, top, top_lp


def op_guidance(lib, raw, s):
    """fvhd_op_dec_guidance on a copy of raw [2 G, V] -> the guided rows [G, V]"""
    x = raw.clone()
    G = x.shape[0] // 2
    nbytes = lib.fvhd_dec_guidance_scratch_bytes(G, x.shape[1])
    scratch = torch.zeros(nbytes, device="cuda", dtype=torch.uint8)
    check(lib.fvhd_op_dec_guidance(stream(), ptr(x), G, x.shape[1], float(s), ptr(scratch), nbytes), "fvhd_op_dec_guidance")
    torch.cuda.synchronize()
    return x[:G].contiguous()


GUIDANCE_TC, GUIDANCE_TU = 9, 6      # prompt and negative-prompt lengths of `guidance_inputs`: the negative half is left-padded by 3 more


def guidance_inputs(m16, G, seed=0, same=False, vocab=4096):
    """prompts as ids, embeddings from the model's table; row g of either half has g % 3 padded positions on the left -> (prompt embeddings,
    mask, negative-prompt embeddings, mask)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(10, vocab, (G, GUIDANCE_TC), generator=g).cuda()
    nids = ids.clone() if same else torch.randint(10, vocab, (G, GUIDANCE_TU), generator=g).cuda()
    mask, nmask = torch.ones_like(ids), torch.ones_like(nids)
    for b in range(G):
        mask[b, :b % 3] = 0
        nmask[b, :b % 3] = 0
    emb = m16.get_input_embeddings()
    with torch.no_grad():
        return emb(ids), mask, emb(nids), nmask


# ---- models: the decode tests' ---------------------------------------------------------------------------------------------------------
DELTA = 0.02         # fp32 logit margin above which our bf16 step must pick the oracle's token (the steps' logit error is ~10x smaller)

CONFIGS = {
    "0.5B": dict(hidden_size=896, num_hidden_layers=2, num_attention_heads=14, num_key_value_heads=2, intermediate_size=4864, tie_word_embeddings=True),
    "1.5B": dict(hidden_size=1536, num_hidden_layers=1, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960, tie_word_embeddings=True),
    "7B": dict(hidden_size=3584, num_hidden_layers=1, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944, tie_word_embeddings=False),
}


def models(name, seed=0, vocab=4096, device="cuda", quantised=False, layers=None):
    """(bf16 model, fp32 oracle on the same bf16-rounded weights); quantised: every 2-D weight of the decoder stack and lm_head holds
    dequantised e4m3 values (codes * scale, exact in bf16): an exact-weight oracle for the 8-bit path"""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(seed)
    kw = dict(CONFIGS[name])
    if layers:
        kw["num_hidden_layers"] = layers
    cfg = Qwen2Config(vocab_size=vocab, max_position_embeddings=4096, rope_theta=1e6, rms_norm_eps=1e-6, **kw)
    m = Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():                                  # biases and norm weights away from their trivial init
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    m16 = m.to(device, torch.bfloat16)
    if quantised:
        from ml_fastvlm_amd import quantize_rows_e4m3
        emb = m16.get_input_embeddings().weight
        with torch.no_grad():
            for p in m16.parameters():
                if p.dim() == 2 and (p is not emb or cfg.tie_word_embeddings):
                    codes, scale = quantize_rows_e4m3(p)
                    p.copy_((codes.float() * scale[:, None]).to(torch.bfloat16))
    ref = Qwen2ForCausalLM(cfg).eval().to(device)
    ref.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    return m16, ref


def prompt(ref, B, T, side, seed=0, draw_on="cuda"):
    """bf16-rounded embeddings and a mask on ref's device, row b with 3 b padded positions; draw_on: the device of the generator (the
    seed lists of the tests were chosen for one or the other)"""
    g = torch.Generator(device=draw_on).manual_seed(seed)
    e = 0.5 * torch.randn(B, T, ref.config.hidden_size, device=draw_on, generator=g)
    e = e.to(torch.bfloat16).float().to(ref.device)
    mask = torch.ones(B, T, device=ref.device, dtype=torch.long)
    for b in range(B):
        npad = 3 * b
        if npad:
            if side == "left":
                mask[b, :npad] = 0
            else:
                mask[b, T - npad:] = 0
    return e, mask


def wide_prompt(ref, B, T, seed=0, distinct=None):
    """B rows with mixed left padding ((5 b) % 13 positions), drawn on ref's device; distinct = n: rows are copies of the first n (row
    b = row b % n)"""
    n = B if distinct is None else distinct
    dev = ref.device
    g = torch.Generator(device=dev).manual_seed(seed)
    e = (0.5 * torch.randn(n, T, ref.config.hidden_size, device=dev, generator=g)).to(torch.bfloat16).float()
    mask = torch.ones(n, T, device=dev, dtype=torch.long)
    for b in range(n):
        mask[b, :(5 * b) % 13] = 0
    idx = torch.arange(B, device=dev) % n
    return e[idx].contiguous(), mask[idx].contiguous()


def agree(ours, ref_seq, scores, delta=DELTA):
    """token-for-token equality of every row up to the oracle's first step with a top-2 margin <= delta; -> steps compared per row"""
    n = []
    for b in range(ref_seq.shape[0]):
        i = 0
        while i < ref_seq.shape[1]:
            top = scores[i][b].float().topk(2).values
            if (top[0] - top[1]).item() <= delta:
                break
            assert i < ours.shape[1] and int(ours[b, i]) == int(ref_seq[b, i]), (b, i, ours[b].tolist(), ref_seq[b].tolist())
            i += 1
        n.append(i)
    return n


# prompt seeds (of `prompt` drawn on the GPU, model seed 1) where the fp32 oracle's top-2 margin exceeds 2 * DELTA at EVERY step of every
# row for 12 new tokens: there bf16 rounding cannot legitimately pick another token, so the outputs must be equal token for token
GREEDY_SEEDS = {"left": [14, 83], "right": [64, 187]}


def tiny_qwen2():
    """a 64-wide one-layer Qwen2ForCausalLM on the CPU, for the checks that run before any device is looked at"""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(vocab_size=64, hidden_size=64, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, intermediate_size=128)
    return Qwen2ForCausalLM(cfg)


# ---- models: the prefill tests' --------------------------------------------------------------------------------------------------------
def qwen2_cfg(hidden=128, layers=2, heads=2, kv=1, inter=256, vocab=512, theta=1e6, head_dim=None):
    from transformers import Qwen2Config
    cfg = Qwen2Config(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
                      num_key_value_heads=kv, max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=False)
    for holder in ("rope_parameters", "rope_scaling"):
        d = getattr(cfg, holder, None)
        if isinstance(d, dict):
            d["rope_theta"] = theta
    if hasattr(cfg, "rope_theta") and getattr(cfg, "rope_theta", None) is not None:
        cfg.rope_theta = theta
    cfg._attn_implementation = "eager"
    return cfg


def qwen2_model(cfg, seed=0):
    from transformers import Qwen2ForCausalLM
    torch.manual_seed(seed)
    m = Qwen2ForCausalLM(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                      # HF's init is N(0, 0.02) with zero biases and unit norms: give every tensor some life
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif "norm" in n:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / p.shape[-1] ** 0.5))
    return m


def prefill_inputs(B, T, H, seed=0, pad="none"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, H, generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    pos = torch.arange(T)[None].repeat(B, 1)
    if pad != "none":
        for b in range(B):
            n = (3 * b + 1) % max(2, T // 3)
            if n == 0:
                continue
            if pad == "left":
                mask[b, :n] = 0
                pos[b] = torch.clamp(torch.arange(T) - n, min=0)         # as prepare_inputs_labels_for_multimodal builds them (0 on padding)
            else:
                mask[b, T - n:] = 0
                pos[b, T - n:] = 0
    return x, mask, pos


def compare_prefill(cfg, B, T, pad, seed, layers_tol):
    """the whole prefill of qwen2_model(cfg, seed) against the `transformers` module in fp32 on the bf16-rounded matrices: residual
    stream, last-position logits, greedy token, KV cache -> (model, context, x, mask, pos, logits, k cache, v cache)"""
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    from oracle import qwen2_oracle as QO
    m = qwen2_model(cfg, seed)
    x, mask, pos = prefill_inputs(B, T, cfg.hidden_size, seed=seed + 10, pad=pad)
    x = bf(x)
    sd = {k: (bf(v) if v.dim() == 2 else v) for k, v in m.state_dict().items()}     # the matrices the library holds are bf16
    m.load_state_dict(sd)
    with torch.no_grad():
        want = m(inputs_embeds=x, attention_mask=mask, position_ids=pos).logits[:, -1]
    _, hidden, kvs = QO.prefill(x, sd, cfg, mask, pos)
    pre = Qwen2Prefill.from_hf(m.to(DEV))
    logits, kc, vc = pre(x.to(DEV, torch.bfloat16), mask.to(DEV), pos.to(DEV), return_kv=True)
    torch.cuda.synchronize()
    assert logits.shape == (B, cfg.vocab_size) and logits.dtype == torch.float32 and torch.isfinite(logits).all()
    valid = mask.bool()
    got_h = pre.hidden_states(B * T).float().cpu().view(B, T, -1)
    rel_h, cos_h, _ = metrics(got_h[valid], hidden[valid])
    rel, cos, _ = metrics(logits, want)
    print(f"prefill H={cfg.hidden_size} L={cfg.num_hidden_layers} B={B} T={T} pad={pad}: residual stream rel-L2 {rel_h:.3e} cos {cos_h:.6f}; "
          f"last-position logits rel-L2 {rel:.3e} cos {cos:.6f}")
    assert rel_h <= layers_tol and cos_h >= 0.9998, (rel_h, cos_h)
    if pad != "right":                               # with right padding position -1 is a padding row: meaningless in the reference too
        assert rel <= 2e-2 and cos >= 0.9995, (rel, cos)
        top2 = want.topk(2, -1).values
        err = (logits.cpu() - want).abs().max(-1).values
        for b in range(B):
            if top2[b, 0] - top2[b, 1] > 2 * err[b]:
                assert int(logits[b].argmax()) == int(want[b].argmax())
    # KV cache: rotated keys and values of the valid positions, in transformers' [B, nkv, T, hd] layer layout
    for l in range(cfg.num_hidden_layers):
        vm = valid[:, None, :, None].expand_as(kvs[l][0])
        rk = metrics(kc[l].float().cpu()[vm], kvs[l][0][vm])[0]
        rv = metrics(vc[l].float().cpu()[vm], kvs[l][1][vm])[0]
        assert rk <= layers_tol and rv <= layers_tol, (l, rk, rv)
    return m, pre, x, mask, pos, logits, kc, vc
