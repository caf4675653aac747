"""The C-ABI library loads and exports every symbol include/fvhd.h declares (no compute without a GPU)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ml_fastvlm_amd import build, _lib
    build.build_library()
    return _lib.load()


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "fvhd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fvhd_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    names = _declared_functions()
    assert len(names) >= 20, names
    raw = ctypes.CDLL(os.path.join(ROOT, "ml_fastvlm_amd", "libfvhd.so"))
    missing = [n for n in names if not hasattr(raw, n)]
    assert not missing, f"declared in fvhd.h but not exported: {missing}"


def test_binding_covers_header(lib):
    # every declared function has ctypes argtypes in the Python stub
    for n in _declared_functions():
        assert getattr(lib, n).argtypes is not None or n in ("fvhd_version", "fvhd_last_error"), n


def test_version_and_error_string(lib):
    # the library reports the FVHD_VERSION of the header it was built from, and the ctypes stub was written against the same major version
    # (round 4 changed exported signatures under an unchanged version number; _lib.load() now refuses a mismatch)
    from ml_fastvlm_amd import _lib
    src = open(os.path.join(ROOT, "include", "fvhd.h")).read()
    header = int(re.search(r"#define\s+FVHD_VERSION\s+(\d+)", src).group(1))
    assert lib.fvhd_version() == header and header // 100 == _lib.ABI_VERSION // 100 and header >= _lib.ABI_VERSION
    assert isinstance(lib.fvhd_last_error(), bytes)


def test_bad_arguments_are_errors_not_crashes(lib):
    h = ctypes.c_void_p()
    assert lib.fvhd_create(ctypes.byref(h), 0, 1000, 1) != 0          # not a multiple of 64
    assert b"multiple of 64" in lib.fvhd_last_error()
    assert lib.fvhd_create(ctypes.byref(h), 0, 1024, 0) != 0
    assert lib.fvhd_finalize_weights(None) != 0
    assert lib.fvhd_encode(None, None, 0, 1, None, 0, None) != 0
    assert lib.fvhd_num_tokens(None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback(lib):
    h = ctypes.c_void_p()
    assert lib.fvhd_create(ctypes.byref(h), 0, 1024, 1) != 0
    assert b"no HIP device" in lib.fvhd_last_error()
    assert not h.value


@pytest.mark.parametrize("C", [96, 192, 384])
def test_ffn_pack_layout(lib, C):
    """fvhd_ffn_pack (host-only): the chunk images are the documented XOR-swizzled LDS byte order, restated here
    independently of the C++ packer."""
    HID, nch, che = 4 * C, 4 * C // 32, 32 * C
    g = torch.Generator().manual_seed(C)
    w1 = torch.randn(HID, C, generator=g).to(torch.bfloat16).float().contiguous()
    w2 = torch.randn(C, HID, generator=g).to(torch.bfloat16).float().contiguous()
    # f16 edge cases of the W2 image (positions the loops below visit): 4 w below the f16 normal range, below half the smallest subnormal,
    # and beyond the largest finite value (the packer saturates where torch's .half() gives inf)
    w2[0, 0], w2[0, 1], w2[0, 2], w2[0, 3] = 1.0e-6, 5.0e-9, -1.0e-6, 3.0e4
    i1 = torch.empty((nch + 1) * che, dtype=torch.bfloat16)
    i2 = torch.empty(nch * che, dtype=torch.bfloat16)
    vp = ctypes.c_void_p
    assert lib.fvhd_ffn_pack(C, vp(w1.data_ptr()), vp(w2.data_ptr()), vp(i1.data_ptr()), vp(i2.data_ptr()), 0) == 0
    assert lib.fvhd_ffn_pack(128, vp(w1.data_ptr()), vp(w2.data_ptr()), vp(i1.data_ptr()), vp(i2.data_ptr()), 0) != 0
    # the half-precision form of the kernel (include/fvhd.h): W1 carries the factor 1/4 (exact in bf16), W2 is IEEE half of 4 W2
    i1 = i1.float() * 4.0
    i2 = i2.view(torch.float16).float() / 4.0
    want2 = (4.0 * w2).half().float().clamp(-65504.0, 65504.0) / 4.0
    assert torch.count_nonzero(i1[nch * che:]) == 0

    def w1_off(row, slot):      # bytes
        if C == 384:
            return row * 768 + ((slot ^ (row & 15)) << 4)
        if C == 192:
            return row * 384 + ((slot ^ ((row >> 1) & 7)) << 4)
        return row * 192 + ((slot ^ ((row >> 2) & 3)) << 4)

    def w2_off(row, slot):
        return row * 64 + ((slot ^ ((row >> 2) & 3)) << 4)

    for ch in (0, 1, nch - 1):
        for row in (0, 5, 17, 31):
            for slot in (0, 3, C // 8 - 1):
                o = ch * che + w1_off(row, slot) // 2
                assert torch.equal(i1[o:o + 8], w1[ch * 32 + row, slot * 8: slot * 8 + 8])
        for n in (0, 7, C - 1):
            for slot in range(4):
                o = ch * che + w2_off(n, slot) // 2
                for e in range(8):
                    pos = slot * 8 + e
                    kb, hf, j = pos >> 4, (pos >> 3) & 1, pos & 7
                    h = 16 * kb + 8 * (j >> 2) + 4 * hf + (j & 3)
                    assert i2[o + e] == want2[n, ch * 32 + h]


def test_split_k_plan_is_host_logic(lib):
    """fvhd_gemm_splitk_plan (pure host code): which residual GEMMs of the tower get their K split - the small-batch shapes do, the benchmark's do not,
    every plan keeps tiles x slices within two workgroups per CU and at least six K steps per slice."""
    want = {(4096, 384, 1536): 1, (1024, 768, 3072): 8, (256, 1536, 6144): 16, (1024, 768, 768): 1, (2048, 1536, 6144): 2,      # B = 1 stages 2 (K < 2048: unsplit) - 4, proj, B = 8 stage 4
            (32768, 768, 3072): 1, (8192, 1536, 6144): 1, (131072, 384, 1536): 1, (8192, 768, 3072): 1,                        # B = 32 / B = 8 stage 3: plenty of tiles
            (4096, 192, 768): 1, (4096, 384, 100): 1, (0, 384, 1536): 1}                                                        # N % 128, K % 64, empty
    for (M, N, K), sp in want.items():
        got = lib.fvhd_gemm_splitk_plan(M, N, K)
        assert got == sp, ((M, N, K), got, sp)
        if got > 1:
            assert -(-M // 128) * (N // 128) * got <= 512 and K % (64 * got) == 0 and K // got >= 384


def test_gemm_kernel_plan_is_host_logic(lib):
    """fvhd_gemm_kernel_plan (version 508, pure host code): the FVHD_GEMM_PLAN_* codes of the header are the stub's, and the query names
    the kernel class of the shapes the dispatch comments name - on a machine without a device the rules are those of 256 CUs."""
    from ml_fastvlm_amd import _lib
    src = open(os.path.join(ROOT, "include", "fvhd.h")).read()
    codes = {n: int(v) for n, v in re.findall(r"#define\s+FVHD_(GEMM_PLAN_[A-Z0-9_]+)\s+(\d+)", src)}
    assert len(codes) == 9 and sorted(codes.values()) == list(range(9))
    assert all(getattr(_lib, n) == v for n, v in codes.items())
    assert _lib.GEMM_PLAN_VERSION == 508 <= lib.fvhd_version() and _lib.gemm_plan_lib() is lib
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        return
    want = {(1, 96, 96, 1, 2): _lib.GEMM_PLAN_V1_NF3_BK32, (256, 384, 96, 2, 2): _lib.GEMM_PLAN_V1_NF4_BK32, (513, 192, 384, 3, 2): _lib.GEMM_PLAN_V1_NF3_BK64,
            (257, 1152, 64, 0, 2): _lib.GEMM_PLAN_V1_NF4_BK64, (131112, 192, 192, 2, 2): _lib.GEMM_PLAN_128X192, (131112, 192, 192, 1, 2): _lib.GEMM_PLAN_V1_NF3_BK64,
            (128, 128, 128, 2, 2): _lib.GEMM_PLAN_V1S, (32768, 128, 128, 0, 2): _lib.GEMM_PLAN_V1S, (32896, 128, 128, 0, 2): _lib.GEMM_PLAN_V1_NF4_BK64,
            (8192, 2048, 128, 2, 2): _lib.GEMM_PLAN_256X128, (7936, 2048, 128, 2, 2): _lib.GEMM_PLAN_V1_NF4_BK64, (11008, 384, 3072, 0, 2): _lib.GEMM_PLAN_256X128,
            (12800, 2304, 128, 0, 2): _lib.GEMM_PLAN_256X256, (12544, 2304, 128, 0, 2): _lib.GEMM_PLAN_256X128,
            (8192, 1024, 3072, 3, 2): _lib.GEMM_PLAN_PINGPONG, (8192, 1024, 3136, 0, 2): _lib.GEMM_PLAN_PINGPONG, (8192, 1024, 3008, 0, 2): _lib.GEMM_PLAN_V1_NF4_BK64,
            (200, 384, 1536, 1, 0): _lib.GEMM_PLAN_V1_NF4_BK64, (200, 384, 1536, 1, 1): _lib.GEMM_PLAN_V1_NF4_BK64, (8, 1024, 896, 0, 0): _lib.GEMM_PLAN_V1_NF4_BK64,
            # refused: K % 32, N % 16, empty, an epilogue that does not exist, output types an epilogue does not have
            (8, 8, 40, 0, 2): -1, (8, 16, 40, 0, 2): -1, (0, 16, 32, 0, 2): -1, (8, 16, 32, 6, 2): -1, (8, 16, 32, -1, 2): -1, (200, 384, 1536, 3, 0): -1,
            (200, 384, 1536, 0, 1): -1, (200, 384, 1536, 1, 3): -1}
    for args, plan in want.items():
        got = lib.fvhd_gemm_kernel_plan(*args)
        assert (got < 0) if plan < 0 else got == plan, (args, got, plan)
