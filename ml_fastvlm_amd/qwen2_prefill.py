"""Qwen2 prefill on hand-written gfx950 kernels - the LLM half of FastVLM's time to first token.

The reference's prefill is `LlavaQwen2ForCausalLM.forward(inputs_embeds=...)` -> `transformers` `Qwen2ForCausalLM.forward`
(`llava/model/language_model/llava_qwen.py:92-103`; `generate`, `:138-143`, enters it for the first token).  `Qwen2Prefill` stands
where that module stands for the prefill step: it is built FROM the module (`from_hf`: same config, weights under the same
state-dict keys), takes the `inputs_embeds` / `attention_mask` / `position_ids` that `prepare_inputs_labels_for_multimodal` (or
`ml_fastvlm_amd.splice.multimodal_splice`) returns, and gives the logits of the last position - what `generate` samples the first
token from - plus, on request, the KV cache in `transformers`' per-layer layout so that the stock decode loop can continue.

    pre = Qwen2Prefill.from_hf(model)                     # model: Qwen2ForCausalLM / LlavaQwen2ForCausalLM on a HIP device
    logits = pre(inputs_embeds, attention_mask, position_ids)           # [B, vocab] fp32

Per decoder layer: RMSNorm -> ONE GEMM for q|k|v (+bias) -> rotary embedding in place -> causal grouped-query flash attention ->
o_proj GEMM with the residual in its epilogue -> RMSNorm -> ONE GEMM for gate|up with silu(gate)*up in its epilogue -> down_proj
GEMM with the residual in its epilogue: 8 launches, all through `libfvhd.so` (`fvhd_llm_*`, include/fvhd.h).  No CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib


class Qwen2Prefill:
    def __init__(self, device_index: int, hidden: int, n_layers: int, n_heads: int, n_kv_heads: int, head_dim: int, intermediate: int,
                 vocab: int, rms_eps: float = 1e-6, rope_theta: float = 1e6):
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.fvhd_llm_create(C.byref(h), device_index, hidden, n_layers, n_heads, n_kv_heads, head_dim, intermediate, vocab,
                                       float(rms_eps), float(rope_theta)), "fvhd_llm_create")
        self._h = h
        self.device = torch.device("cuda", device_index)
        self.hidden, self.n_layers, self.n_heads, self.n_kv_heads, self.head_dim = hidden, n_layers, n_heads, n_kv_heads, head_dim
        self.intermediate, self.vocab = intermediate, vocab
        self.tie_word_embeddings = None           # from_hf records the config's flag (the decode's input embedding depends on it)
        self.weight_format = "bf16"               # set_weight_format: "fp8_e4m3" = the packed matrices as e4m3 codes + one scale per row,
                                                  # "mxfp4" = as e2m1 codes + one power-of-two scale per 32 elements of a row
        self._tensors_set = 0

    # ---- construction from the reference's module -------------------------------------------------------------------------------
    @classmethod
    def from_hf(cls, model, device: Optional[torch.device] = None, weights: str = "bf16") -> "Qwen2Prefill":
        """model: a `transformers` Qwen2ForCausalLM (or the reference's LlavaQwen2ForCausalLM, whose decoder stack it is).
        weights: "bf16" (the default), or "fp8_e4m3" - every matrix of the decoder stack and lm_head stored as OCP e4m3 codes with one
        power-of-two scale per output row (`quantize_rows_e4m3`), quantised on the device as it is packed: half the bytes held and half the
        bytes a decode step streams; or "mxfp4" - the same matrices as OCP MXFP4 (`quantize_blocks_mxfp4`: e2m1 codes, one power-of-two
        scale per 32 elements of a row, 4.25 bits per weight; a coarse format).  Activations, the KV cache and the arithmetic (bf16 MFMA,
        fp32 accumulation) stay what they are."""
        _lib.weight_format_code(weights)
        cfg = model.config
        dev = torch.device(device) if device is not None else next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("Qwen2Prefill (MI355X): the model must be on a HIP device - this path has no CPU implementation")
        scaling = getattr(cfg, "rope_scaling", None) or getattr(cfg, "rope_parameters", None)
        rope_type = (scaling or {}).get("rope_type", (scaling or {}).get("type", "default")) if isinstance(scaling, dict) else "default"
        if rope_type not in ("default", None):
            raise NotImplementedError(f"rope type {rope_type!r}: only the default rotary embedding of Qwen2 is implemented")
        if getattr(cfg, "use_sliding_window", False):
            raise NotImplementedError("sliding-window attention is off in every FastVLM checkpoint and is not implemented")
        theta = getattr(cfg, "rope_theta", None)
        if theta is None and isinstance(scaling, dict):
            theta = scaling.get("rope_theta")
        head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        self = cls(dev.index if dev.index is not None else torch.cuda.current_device(), cfg.hidden_size, cfg.num_hidden_layers,
                   cfg.num_attention_heads, cfg.num_key_value_heads, head_dim, cfg.intermediate_size, cfg.vocab_size,
                   getattr(cfg, "rms_norm_eps", 1e-6), float(theta if theta is not None else 1e6))
        mpe = getattr(cfg, "max_position_embeddings", None)
        if mpe:                                   # rows of the rotary table; positions beyond it are computed in the kernel, never clamped
            _lib.check(_lib.load().fvhd_llm_set_max_positions(self._h, int(mpe)), "fvhd_llm_set_max_positions")
        self.tie_word_embeddings = bool(getattr(cfg, "tie_word_embeddings", False))
        self.set_weight_format(weights)
        self.load_state_dict(model.state_dict())
        return self

    def set_weight_format(self, weights: str) -> None:
        """"bf16", "fp8_e4m3" or "mxfp4" (`fvhd_llm_set_weight_format`): before the first tensor is set - the matrices are quantised as they arrive"""
        code = _lib.weight_format_code(weights)
        if weights == self.weight_format:
            return
        if self._tensors_set:
            raise _lib.FvhdError(f"Qwen2Prefill.set_weight_format({weights!r}): {self._tensors_set} tensors were already set as "
                                 f"{self.weight_format} - choose the format before the first tensor (from_hf(model, weights=...))")
        lib = _lib.w4_lib() if weights in _lib.MX_WEIGHT_FORMATS else _lib.w8_lib()
        _lib.check(lib.fvhd_llm_set_weight_format(self._h, code), "fvhd_llm_set_weight_format")
        self.weight_format = weights

    @property
    def weight_bytes(self) -> int:
        """device bytes of the packed weights (matrices, row scales, norm weights, biases)"""
        n = C.c_size_t(0)
        _lib.check(_lib.w8_lib().fvhd_llm_weight_bytes(self._h, C.byref(n)), "fvhd_llm_weight_bytes")
        return int(n.value)

    def _matrix_shape(self, matrix: int):
        qkvw = (self.n_heads + 2 * self.n_kv_heads) * self.head_dim
        return {_lib.MAT_QKV: (qkvw, self.hidden), _lib.MAT_O: (self.hidden, self.n_heads * self.head_dim),
                _lib.MAT_GATE_UP: (2 * self.intermediate, self.hidden), _lib.MAT_DOWN: (self.hidden, self.intermediate),
                _lib.MAT_LM_HEAD: (self.vocab, self.hidden)}[matrix]

    def packed_mxfp4(self, layer: int, matrix: int):
        """tests: one packed matrix of an "mxfp4" context in plain order -> (codes u8 [N, K / 2], scales u8 [N, K / 32]), the layout of
        `quantize_blocks_mxfp4`; matrix as for `packed_e4m3`"""
        N, K = self._matrix_shape(matrix)
        codes = torch.empty((N, K // 2), device=self.device, dtype=torch.uint8)
        scales = torch.empty((N, K // 32), device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            _lib.check(_lib.w4_lib().fvhd_llm_debug_packed_mxfp4(self._h, int(layer), int(matrix), _lib.ptr(codes), _lib.ptr(scales),
                                                                 _lib.stream_ptr(self.device)), "fvhd_llm_debug_packed_mxfp4")
        return codes, scales

    def packed_e4m3(self, layer: int, matrix: int):
        """tests: one packed matrix of an "fp8_e4m3" context in plain [N, K] order -> (codes float8_e4m3fn [N, K], scale fp32 [N]);
        matrix: `_lib.MAT_QKV` (q | k | v rows), `MAT_O`, `MAT_GATE_UP` (gate / up rows interleaved), `MAT_DOWN`, `MAT_LM_HEAD`"""
        N, K = self._matrix_shape(matrix)
        codes = torch.empty((N, K), device=self.device, dtype=torch.uint8)
        scale = torch.empty((N,), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.w8_lib().fvhd_llm_debug_packed_e4m3(self._h, int(layer), int(matrix), _lib.ptr(codes), _lib.ptr(scale),
                                                                _lib.stream_ptr(self.device)), "fvhd_llm_debug_packed_e4m3")
        return codes.view(torch.float8_e4m3fn), scale

    def load_state_dict(self, sd) -> None:
        """The decoder-stack tensors of a (Llava)Qwen2ForCausalLM state dict; `lm_head.weight` falls back to the embedding table
        (tie_word_embeddings).  Everything else in the dict (vision tower, projector) is ignored."""
        lib = _lib.load()
        seen_head = False
        for key, t in sd.items():
            k = key[6:] if key.startswith("model.") else key
            if not (k.startswith("layers.") or k == "norm.weight" or key == "lm_head.weight"):
                continue
            if k.startswith("layers.") and not any(k.endswith(s) for s in self._LAYER_SUFFIXES):
                continue
            seen_head |= key == "lm_head.weight"
            self._set(lib, key, t)
        if not seen_head:
            emb = sd.get("model.embed_tokens.weight", sd.get("embed_tokens.weight"))
            if emb is None:
                raise KeyError("neither lm_head.weight nor model.embed_tokens.weight in the state dict")
            self._set(lib, "lm_head.weight", emb)
        _lib.check(lib.fvhd_llm_finalize(self._h), "fvhd_llm_finalize")

    _LAYER_SUFFIXES = ("input_layernorm.weight", "post_attention_layernorm.weight", "self_attn.q_proj.weight", "self_attn.q_proj.bias",
                       "self_attn.k_proj.weight", "self_attn.k_proj.bias", "self_attn.v_proj.weight", "self_attn.v_proj.bias",
                       "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")

    def _set(self, lib, key: str, t: torch.Tensor) -> None:
        """A tensor that already lives on this context's device is packed by ONE device-to-device copy (`fvhd_llm_set_tensor_device`:
        matrices as bf16, vectors as fp32 - converted on the device when the module holds another dtype); only host tensors take the
        host path.  (Round 3 moved every tensor device -> CPU -> temporary -> device: 15 GB through the host for the 7B model.)  Note the
        footprint: the packed copy (q|k|v concatenated, gate / up interleaved, bf16) lives NEXT to the module's own weights, which the
        stock decode loop keeps using - 2x the LLM's weight bytes on the device (0.99 GB / 15.2 GB more for Qwen2-0.5B / 7B)."""
        t = t.detach()
        self._tensors_set += 1
        shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
        if t.device.type == "cuda" and t.device == self.device:
            want = torch.bfloat16 if t.dim() == 2 else torch.float32
            d = t.to(want).contiguous()
            with torch.cuda.device(self.device):
                _lib.check(lib.fvhd_llm_set_tensor_device(self._h, key.encode(), C.c_void_p(d.data_ptr()), _lib.dtype_code(want), shape, t.dim(),
                                                          _lib.stream_ptr(self.device)), f"fvhd_llm_set_tensor_device({key})")
            if d is not t and d.data_ptr() != t.data_ptr():
                d.record_stream(torch.cuda.current_stream(self.device))      # the temporary outlives the enqueued copy
            return
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            t = t.float()
        t = t.to("cpu").contiguous()
        _lib.check(lib.fvhd_llm_set_tensor(self._h, key.encode(), C.c_void_p(t.data_ptr()), _lib.dtype_code(t.dtype), shape, t.dim()),
                   f"fvhd_llm_set_tensor({key})")

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.load().fvhd_llm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the prefill ---------------------------------------------------------------------------------------------------------------
    def reserve(self, batch: int, seq_len: int) -> None:
        """size the workspace now (growth synchronises the device and is refused during stream capture)"""
        _lib.check(_lib.load().fvhd_llm_reserve(self._h, int(batch), int(seq_len)), "fvhd_llm_reserve")

    def _check(self, inputs_embeds, attention_mask, position_ids):
        if not isinstance(inputs_embeds, torch.Tensor) or inputs_embeds.dim() != 3 or inputs_embeds.shape[2] != self.hidden \
                or inputs_embeds.shape[0] < 1 or inputs_embeds.shape[1] < 1:
            raise ValueError(f"expected inputs_embeds of shape [B, T, {self.hidden}], got "
                             f"{tuple(inputs_embeds.shape) if isinstance(inputs_embeds, torch.Tensor) else type(inputs_embeds)}")
        x = inputs_embeds.to(self.device).contiguous()
        if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            x = x.float()
        B, T = x.shape[:2]
        am = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, T):
                raise ValueError(f"attention_mask must be [B, T] = {(B, T)}, got {tuple(attention_mask.shape)}")
            am = (attention_mask.to(self.device) != 0).to(torch.uint8).contiguous()
        pos = None
        if position_ids is not None:
            if tuple(position_ids.shape) != (B, T):
                raise ValueError(f"position_ids must be [B, T] = {(B, T)}, got {tuple(position_ids.shape)}")
            pos = position_ids.to(device=self.device, dtype=torch.int64).contiguous()
        return x, am, pos

    @torch.no_grad()
    def __call__(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
                 return_kv: bool = False, out: Optional[torch.Tensor] = None):
        """-> logits [B, vocab] fp32 of the last position; with return_kv also (k, v): bf16 [n_layers, B, n_kv_heads, T, head_dim]."""
        x, am, pos = self._check(inputs_embeds, attention_mask, position_ids)
        B, T = x.shape[:2]
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, self.vocab) or out.dtype != torch.float32
                                or out.device != self.device or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous fp32 tensor [{B}, {self.vocab}] on {self.device} (its raw pointer goes to the kernel)")
        logits = out if out is not None else torch.empty((B, self.vocab), device=self.device, dtype=torch.float32)
        kc = vc = None
        if return_kv:
            kc = torch.empty((self.n_layers, B, self.n_kv_heads, T, self.head_dim), device=self.device, dtype=torch.bfloat16)
            vc = torch.empty_like(kc)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().fvhd_llm_prefill(self._h, _lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(am), _lib.ptr(pos), B, T,
                                                    _lib.ptr(logits), _lib.ptr(kc), _lib.ptr(vc), _lib.stream_ptr(self.device)), "fvhd_llm_prefill")
        self._last_rows = (B, T)                                 # what score_rows may score ...
        self._last_call = object()                               # ... and which call left them (a token: `Qwen2Generator.score_last` compares it)
        return (logits, kc, vc) if return_kv else logits

    @property
    def workspace_generation(self) -> int:
        """increments whenever the library replaced its workspace (a graph the caller captured before stays valid - the old workspace is
        kept alive - but only a re-capture uses the new one)"""
        return int(_lib.load().fvhd_llm_workspace_generation(self._h))

    # ---- scoring given tokens -----------------------------------------------------------------------------------------------------
    def score_reserve(self, rows: int) -> None:
        """size the score scratch for batch * T = `rows` rows now (growth synchronises the device and is refused during stream capture)"""
        _lib.check(_lib.score_lib().fvhd_llm_score_reserve(self._h, int(rows)), "fvhd_llm_score_reserve")

    @torch.no_grad()
    def score_rows(self, targets: torch.Tensor, out: Optional[torch.Tensor] = None, lse_out: Optional[torch.Tensor] = None):
        """The rows of the LAST prefill / start / extend of this context, still in its workspace (`fvhd_llm_score`): targets int64 [B, T]
        on the device, targets[b][t] = the id whose probability under the distribution PREDICTED AT position t is wanted (the caller
        shifts: `score_targets`), negative = ignore -> (logprob fp32 [B, T], lse fp32 [B, T]), both indexed by the predicting position.
        logprob is 0.0 at an ignored target and NaN at a target >= vocab.  Final norm of all rows, lm_head and the log-softmax in one
        kernel: no [B * T, vocab] tensor.  out / lse_out: contiguous fp32 [B, T] buffers to write into (a captured call)."""
        if not isinstance(targets, torch.Tensor) or targets.dim() != 2 or targets.dtype != torch.long:
            raise ValueError(f"score_rows: targets must be an int64 tensor [B, T], got "
                             f"{(targets.dtype, tuple(targets.shape)) if isinstance(targets, torch.Tensor) else type(targets)}")
        want = getattr(self, "_last_rows", None)
        if want is not None and tuple(targets.shape) != want:
            raise ValueError(f"score_rows: targets are {tuple(targets.shape)}, the last prefill / start / extend of this context ran [B, T] = {want}")
        t = targets.to(self.device).contiguous()
        for name, buf in (("out", out), ("lse_out", lse_out)):
            if buf is not None and (buf.dtype != torch.float32 or buf.device != self.device or buf.shape != t.shape or not buf.is_contiguous()):
                raise ValueError(f"score_rows: {name} must be a contiguous fp32 tensor {tuple(t.shape)} on {self.device}")
        lp = out if out is not None else torch.empty(t.shape, device=self.device, dtype=torch.float32)
        lse = lse_out if lse_out is not None else torch.empty(t.shape, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.score_lib().fvhd_llm_score(self._h, _lib.ptr(t), _lib.ptr(lp), _lib.ptr(lse), _lib.stream_ptr(self.device)), "fvhd_llm_score")
        return lp, lse

    @torch.no_grad()
    def score(self, inputs_embeds: torch.Tensor, labels: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
              position_ids: Optional[torch.Tensor] = None):
        """transformers' `forward(labels=...)` per token: `labels` [B, T] is aligned with the inputs and shifted inside ->
        (token_logprobs fp32 [B, T], lse fp32 [B, T]); entry [b][t] = log p(labels[b][t] | tokens < t) and the log-sum-exp of the logits
        it was read from.  token_logprobs is 0 at [b][0], wherever the label is -100 (any negative id) and wherever attention_mask (of the
        token or of the position before it) is 0; lse[b][0] = 0.  -token_logprobs.sum() / (scored tokens) is the reference's loss."""
        if not isinstance(labels, torch.Tensor) or labels.dim() != 2 or tuple(labels.shape) != tuple(inputs_embeds.shape[:2]):
            raise ValueError(f"score: labels must be [B, T] = {tuple(inputs_embeds.shape[:2])}, got "
                             f"{tuple(labels.shape) if isinstance(labels, torch.Tensor) else type(labels)}")
        targets = score_targets(labels.to(self.device), None if attention_mask is None else attention_mask.to(self.device))
        self(inputs_embeds, attention_mask, position_ids)
        return tuple(label_aligned(t) for t in self.score_rows(targets))

    def hidden_states(self, rows: int) -> torch.Tensor:
        """tests: the residual stream after the last decoder layer of the previous prefill, [rows, hidden] bf16"""
        out = torch.empty((rows, self.hidden), device=self.device, dtype=torch.bfloat16)
        _lib.check(_lib.load().fvhd_llm_debug_hidden(self._h, _lib.ptr(out), rows, _lib.stream_ptr(self.device)), "fvhd_llm_debug_hidden")
        return out


def score_targets(labels: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transformers' label shift as the targets of `score_rows` (pure torch, any device): labels [B, T] aligned with the inputs ->
    targets int64 [B, T], targets[b][t] = labels[b][t + 1] - the token position t predicts - and -100 (ignore) at t = T - 1, where the
    label is negative, and where attention_mask is 0 at t + 1 (a padding token is not scored) or at t (a padding position predicts
    nothing: the first real token of a left-padded row has no prefix, like token 0 of an unpadded one)."""
    if labels.dim() != 2:
        raise ValueError(f"score_targets: labels must be [B, T], got {tuple(labels.shape)}")
    if attention_mask is not None and tuple(attention_mask.shape) != tuple(labels.shape):
        raise ValueError(f"score_targets: attention_mask must be [B, T] = {tuple(labels.shape)}, got {tuple(attention_mask.shape)}")
    lab = labels.long()
    tgt = torch.full_like(lab, -100)
    tgt[:, :-1] = lab[:, 1:]
    tgt[tgt < 0] = -100
    if attention_mask is not None:
        keep = attention_mask != 0
        ok = keep.clone()
        ok[:, :-1] &= keep[:, 1:]
        tgt[~ok] = -100
    return tgt.contiguous()


def label_aligned(per_position: torch.Tensor) -> torch.Tensor:
    """a [B, T] result indexed by the PREDICTING position -> indexed by the predicted token: entry [b][t] = input [b][t - 1], 0 at t = 0"""
    return torch.cat([torch.zeros_like(per_position[:, :1]), per_position[:, :-1]], 1)


def quantize_rows_e4m3(w: torch.Tensor):
    """The library's 8-bit weight recipe in plain torch (any device): w [N, K] -> (codes torch.float8_e4m3fn [N, K], scale fp32 [N]), row n
    standing for codes[n] * scale[n].  scale = 2^ceil(log2(amax_row / 448)), evaluated exactly from amax's exponent and mantissa (amax =
    m 2^e, m in [0.5, 1): the exponent is e - 9, + 1 when m > 7/8) and kept >= 2^-126; an all-zero row gets scale 1.  codes = w / scale
    (exact: a power of two) rounded to nearest even by torch's conversion; amax / scale lies in (224, 448], so nothing saturates, and
    codes * scale is exactly representable in bf16."""
    if w.dim() != 2:
        raise ValueError(f"quantize_rows_e4m3 takes a matrix [N, K], got {tuple(w.shape)}")
    wf = w.detach().float()
    amax = wf.abs().amax(1)
    mant, exp = torch.frexp(amax)
    se = (exp - 9 + (mant > 0.875).to(exp.dtype)).clamp(min=-126)
    pow2 = ((se.to(torch.int32) + 127) << 23).view(torch.float32)         # 2^se from its bit pattern (torch.ldexp is inexact on some devices)
    scale = torch.where(amax > 0, pow2, torch.ones_like(amax))
    return (wf / scale[:, None]).to(torch.float8_e4m3fn), scale


def dequantize_rows_e4m3(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """codes * scale as fp32 [N, K] (exact; for power-of-two scales every value is a bf16 value)"""
    return codes.float() * scale.float()[:, None]


E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # the magnitudes of the OCP e2m1 codes, by index (bits 2..0; bit 3 = sign)


def quantize_blocks_mxfp4(w: torch.Tensor):
    """The library's 4-bit weight recipe in plain torch (any device): w [N, K], K % 32 == 0, rounded to bf16 first (the library's matrices
    are bf16) -> (codes u8 [N, K / 2], scales u8 [N, K / 32]).  Element k of a row is in byte k / 2, even k in the low nibble; a code is
    sign (bit 3) + an index into E2M1_GRID; scale byte E of a block of 32 consecutive k stands for 2^(E - 127).
    Per block: se = ceil(log2(amax / 6)) evaluated exactly from amax's bf16 bit pattern (amax = m 2^e, m in [1, 2): e - 2 + (m > 1.5)),
    clamped to [-125, 125], 0 for an all-zero block, E = se + 127.  codes = |w| / 2^se (exact) to the nearest grid value, a tie to the even
    index, above 6 saturating (possible only at the upper clamp); the sign bit is w's own, so a small negative becomes -0.  amax / 2^se lies
    in (3, 6] and code * scale is exactly a bf16 value.  A coarse format: about 0.12 relative L2 error on a Gaussian matrix."""
    if w.dim() != 2 or w.shape[1] % 32:
        raise ValueError(f"quantize_blocks_mxfp4 takes a matrix [N, K] with K % 32 == 0, got {tuple(w.shape)}")
    N, K = w.shape
    bits = w.detach().to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int32) & 0xffff
    mag = (bits & 0x7fff).view(N, K // 32, 32)
    am = mag.amax(-1)
    se = ((am >> 7) - 127 - 2 + ((am & 0x7f) > 0x40).to(torch.int32)).clamp(-125, 125)
    se = torch.where(am > 0, se, torch.zeros_like(se))
    inv = ((127 - se) << 23).view(torch.float32)                          # 2^-se from its bit pattern
    a = (mag << 16).view(torch.float32) * inv[..., None]
    idx = ((a > 0.25).to(torch.int32) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0)).view(N, K)
    code = ((bits >> 15) << 3) | idx
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)
    return codes, (se + 127).to(torch.uint8)


def dequantize_blocks_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """code * 2^(E - 127) as bf16 [N, K] (exact; a code with the sign bit and index 0 gives -0); scale bytes 1 .. 254"""
    N, K = codes.shape[0], codes.shape[1] * 2
    c = codes.to(torch.int32)
    code = torch.stack([c & 0xf, c >> 4], -1).view(N, K)
    grid = torch.tensor(E2M1_GRID, device=codes.device, dtype=torch.float32)
    val = grid[code & 7]
    val = torch.where((code & 8) != 0, -val, val)
    scale = (scales.to(torch.int32) << 23).view(torch.float32)
    return (val.view(N, K // 32, 32) * scale[..., None]).view(N, K).to(torch.bfloat16)


def kv_to_dynamic_cache(k: torch.Tensor, v: torch.Tensor):
    """(k, v) of `Qwen2Prefill(..., return_kv=True)` -> a `transformers.DynamicCache` the stock decode loop continues from."""
    from transformers import DynamicCache
    cache = DynamicCache()
    for layer in range(k.shape[0]):
        cache.update(k[layer], v[layer], layer)
    return cache


def rope_table(positions: int, head_dim: int, theta: float = 1e6, device="cpu") -> torch.Tensor:
    """(cos, sin) table [positions, head_dim / 2, 2] fp32 exactly as the library builds it (and as Qwen2RotaryEmbedding.forward does:
    inv_freq = theta^(-2i / head_dim) in fp32, angle = position * inv_freq in fp32) - for the single-op tests."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    ang = torch.arange(positions, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], -1).contiguous().to(device)
