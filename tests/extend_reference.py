"""TEST INFRASTRUCTURE ONLY - references for extending a started KV cache (csrc/llm_extend.hip), built on tests/prefill_reference.py:
the attention of a chunk over `past + chunk` keys is the causal attention of the CONCATENATED sequence restricted to the chunk's rows
(`attention_ref`, fp64), so nothing about the kernel is restated here; plus plain-Python models of the rewind and of the default positions,
and the helpers that lay a concatenated sequence out as the op sees it (chunk rows + strided caches).

PINNING: tests/test_extend_reference.py checks the restriction against a direct computation, the models against hand-made cases, and the
headroom of every input family the GPU tests use (prefill_reference.flash_model, whose 64-key tiles are aligned to slot 0 like the
kernel's, on rows >= P: err / bound <= 0.5)."""
from __future__ import annotations

import torch

import prefill_reference as R
from llm_testlib import SENT

# (P, T) of the op tests: a one-token cache and chunk, the chunk ending at / starting on / straddling a 64-key tile edge, more than one
# 128-query workgroup on a past that is no multiple of the tile, whole tiles of past under a full workgroup, one query behind a long past,
# a long chunk behind a short past
PT = [(1, 1), (63, 17), (64, 64), (65, 17), (130, 129), (192, 128), (257, 1), (5, 200)]
HEADS = [(64, 14, 2), (128, 28, 4), (64, 4, 2)]              # hd, nh, nkv


def chunk_rows(qkv_full, B, P, T):
    """packed rows of the concatenated sequence [B * (P + T), width] -> the chunk's rows [B * T, width] (a contiguous copy)"""
    N = P + T
    return qkv_full.view(B, N, -1)[:, P:].reshape(B * T, -1).contiguous()


def attention_extend_ref(qkv_full, key_valid_full, B, P, T, nh, nkv, hd):
    """fp64 reference of the op: attention_ref on the concatenated [past | chunk] sequence, rows >= P ->
    (out [B, T, nh, hd] fp64, empty [B, T] bool: the chunk query has no visible key and the op writes zeros)"""
    q, k, v = R.split_heads(qkv_full, B, P + T, nh, nkv, hd)
    out, empty = R.attention_ref(q, k, v, key_valid_full)
    return out[:, P:], empty[:, P:]


def flash_extend_model(qkv_full, key_valid_full, B, P, T, nh, nkv, hd):
    """prefill_reference.flash_model on the concatenated sequence, rows >= P: its 64-key tiles start at slot 0, the arithmetic the extend
    kernel is required to have -> [B, T, nh, hd] bf16"""
    q, k, v = R.split_heads(qkv_full, B, P + T, nh, nkv, hd)
    return R.flash_model(q, k, v, key_valid_full)[:, P:]


def caches(qkv_full, B, N, nh, nkv, hd, cap, cache_batch):
    """the k / v heads of the concatenated rows in slots [0, N) of sentinel-filled strided caches -> (k, v) bf16 [cache_batch, nkv, cap, hd];
    every slot >= N and every row >= B holds the sentinel (1.23e36): a wrong stride reads it"""
    dev = qkv_full.device
    x = qkv_full.view(B, N, nh + 2 * nkv, hd)
    out = []
    for lo in (nh, nh + nkv):
        c = torch.full((cache_batch, nkv, cap, hd), SENT, device=dev, dtype=torch.int16).view(torch.bfloat16)
        c[:B, :, :N] = x[:, :, lo:lo + nkv].transpose(1, 2)
        out.append(c)
    return out[0], out[1]


def cache_mask(key_valid_full, B, N, cap, cache_batch, device):
    """the decode mask [cache_batch, cap]: key_valid (or ones) in [0, N), ONES behind it and in the spare rows - a kernel that read a key
    >= P + T, or another row's mask, would find it valid"""
    m = torch.ones(cache_batch, cap, device=device, dtype=torch.uint8)
    if key_valid_full is not None:
        m[:B, :N] = key_valid_full
    return m


def rewind_model(mask, positions, length, keep):
    """fvhd_llm_cache_rewind on host tensors: mask uint8 [rows, cap], positions int64 [rows], length int, keep: ints ->
    (mask, positions, length, error word).  A keep outside [0, length] changes nothing and gives error word 4."""
    mask, positions = mask.clone(), positions.clone()
    keep = [int(k) for k in keep]
    if any(k < 0 or k > length for k in keep):
        return mask, positions, length, 4
    for b, k in enumerate(keep):
        positions[b] -= int((mask[b, k:length] != 0).sum())
        mask[b, k:length] = 0
    return mask, positions, max(keep), 0


def extend_positions_model(next_positions, chunk_valid, T):
    """pos[b][t] = next[b] + (valid chunk tokens of row b before t); chunk_valid [B, T] or None (all valid) -> int64 [B, T]"""
    B = next_positions.shape[0]
    valid = torch.ones(B, T, dtype=torch.long) if chunk_valid is None else (chunk_valid != 0).long().cpu()
    before = valid.cumsum(1) - valid
    return next_positions.cpu().long()[:, None] + before


def op_families(P, T):
    """(name, B, pad) of every input family of the op test at (P, T): "planted" and "holes" carry four forms, one per row; "left" once
    with the padding inside the past and once reaching into the chunk (the chunk queries in front of the first valid key are all-masked
    rows); "holes" (whole 64-key tiles invalid) where the sequence has the tiles"""
    N = P + T
    fams = [("plain", 1, None), ("qscale", 3, None), ("ascending", 1, None), ("descending", 1, None), ("planted", 4, None)]
    if P > 1:
        fams.append(("left", 3, [1, max(1, P // 2), P - 1]))
    if T > 1:
        fams.append(("left", 3, [P, P + T // 2, N - 1]))
        fams.append(("right", 3, [1, max(1, T // 2), T - 1]))
    if N >= 200:
        fams.append(("holes", 4, None))
    return fams
