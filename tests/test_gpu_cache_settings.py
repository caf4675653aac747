"""The SETTINGS of the Qwen2 context - logits processors, sampling, log-probabilities - crossed with the cache calls (include/fvhd.h "LLM
logits processors", "LLM sampling", "LLM log-probabilities"): scripts g - m of tests/cache_scripts.py on the library, side by side with
the host model (tests/cache_model.py), and the pair sweep - every ordered pair of ten calls behind a start under each of four settings,
where the library's outcome (ran or refused, the reason, length, error word, run batch, whether step(None) is still allowed) must be the
model's: nothing runs that the header does not define.

No tolerance is new: raw logits under the budget of cache_scripts (rel-L2 <= 2e-2, cos >= 0.9995 per row), log-probabilities under the
derived bound of tests/logprobs_reference.py, everything else equality of bits or of host-visible state.  `twin` = a second generator on a
context of its own with the same weights: the route the first is compared with."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cache_model as CM  # noqa: E402
import cache_scripts as S  # noqa: E402
import llm_testlib as L  # noqa: E402
import logprobs_reference as LR  # noqa: E402
from cache_model import CacheModel, Refused  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = {"bf16": "bf16", "e4m3": "fp8_e4m3", "mxfp4": "mxfp4"}


@functools.lru_cache(maxsize=None)
def _contexts(fmt):
    """(the model, the oracle, two prefill contexts of the same weights) per weight format, made once"""
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, ref = S.stand_in("0.5B", fmt, device="cuda")
    return m16, ref, [Qwen2Prefill.from_hf(m16, weights=FORMATS[fmt]) for _ in range(2)]


def _sides(key, fmt="bf16", batch=None, capacity=None):
    """(side, twin): two generators on two contexts, each with the verify and reorder scratch (reserving them changes no state)"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    _, b, cap = S.SETTINGS_SCRIPTS[key]
    m16, ref, pres = _contexts(fmt)
    out = []
    for i, pre in enumerate(pres):
        gen = Qwen2Generator.from_hf(m16, batch or b, capacity or cap, prefill=pre, weights=pre.weight_format)
        gen.set_sampling(False)
        gen.set_logits_processors()
        gen.spec_reserve(16, 64)
        gen.beam_reserve()
        out.append(S.GpuSide(ref, gen, name=f"{key}{' twin' if i else ''} 0.5B{'' if fmt == 'bf16' else ' ' + fmt}"))
    return out


def _seed(key, fmt="bf16"):
    return S.SETTINGS_SEEDS[(key, fmt)]


# ---- g, h, i: the processors' history ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "e4m3", "mxfp4"])
def test_g_processors_on_the_straight_path_through_the_model(fmt):
    side, twin = _sides("g", fmt)
    S.script_g(side, twin, seed=_seed("g", fmt))


def test_h_rows_a_smaller_start_did_not_reset_begin_empty():
    side, twin = _sides("h")
    S.script_h(side, twin, seed=_seed("h"))


def test_i_a_step_with_processors_off_appends_nothing():
    side, twin = _sides("i")
    S.script_i(side, twin, seed=_seed("i"))


# ---- j: refusals change nothing -----------------------------------------------------------------------------------------------------------------
def _abi_refusals(side, phase):
    """the refused calls of script j through the C ABI: a non-zero return code, fvhd_last_error names the reason, nothing has changed"""
    from ml_fastvlm_amd import _lib
    gen, lib = side.gen, _lib.lookup_lib()
    _lib.extend_lib(), _lib.beam_lib()
    h, st, dev = gen.pre._h, _lib.stream_ptr(gen.device), gen.device
    drafts = torch.tensor([1, 2, 3, 4], device=dev, dtype=torch.long)
    out = torch.zeros(4, device=dev, dtype=torch.long)
    eos = (C.c_int32 * 1)(0)
    chunk = torch.zeros(1, S.J_T, side.ref.config.hidden_size, device=dev, dtype=torch.bfloat16)
    keep = torch.tensor([S.J_P], device=dev, dtype=torch.int32)
    src = torch.zeros(2, device=dev, dtype=torch.long)
    verify = lambda: lib.fvhd_llm_verify(h, _lib.ptr(drafts), 5, None, None, None, st)      # noqa: E731
    begin = lambda: lib.fvhd_llm_lookup_begin(h, None, 0, C.cast(eos, C.c_void_p), 0, 4, _lib.ptr(out), st)      # noqa: E731
    if phase == "processors":
        calls = [("fvhd_llm_extend", CM.NO_CHUNK_IDS, lambda: lib.fvhd_llm_extend(h, _lib.ptr(chunk), _lib.dtype_code(chunk.dtype), None, None, S.J_T, None, None, st)),
                 ("fvhd_llm_cache_rewind", CM.NOT_REWOUND, lambda: lib.fvhd_llm_cache_rewind(h, _lib.ptr(keep), st)),
                 ("fvhd_llm_verify", CM.NOT_MAINTAINED, verify), ("fvhd_llm_lookup_begin", CM.NOT_MAINTAINED, begin),
                 ("fvhd_llm_cache_gather", CM.NOT_REORDERED, lambda: lib.fvhd_llm_cache_gather(h, _lib.ptr(src), 1, 2, st))]
    else:
        calls = [("fvhd_llm_verify", CM.GREEDY_ONLY, verify), ("fvhd_llm_lookup_begin", CM.GREEDY_ONLY, begin),
                 ("fvhd_llm_lookup_step", CM.GREEDY_ONLY, lambda: lib.fvhd_llm_lookup_step(h, 5, 2, st))]
    for who, reason, call in calls:
        rc = call()
        err = lib.fvhd_last_error() if rc else b""
        print(f"{side.name} {phase}: {who} -> {rc} {err[:110]!r}")
        assert rc != 0, (phase, who, "was not refused")
        assert who.encode() in err and reason.encode() in err, (who, err)
        side._check_state()


def test_j_refusals_change_nothing():
    side, twin = _sides("j")
    S.script_j(side, twin, seed=_seed("j"), abi=_abi_refusals)


# ---- k: the draw under moved state --------------------------------------------------------------------------------------------------------------
def _draw_check(side, lg, ids):
    """behind the fork 1 -> 3: row r's id is the sampler op's on that row's logits with the model's (seed, r, n); the three rows - equal
    logits - do not all draw row 0's stream, and n is the moved length (the draw at n - 1 is another)"""
    lib = L._lib.sampling_lib()
    m, w = side.model, side.warp
    keys = [m.draw_key(r, add=0) for r in range(m.run_batch)]
    n = keys[0][2]
    assert [k[1] for k in keys] == [0, 1, 2] and all(k[2] == n == side.gen.length() for k in keys)
    want, info = L.sample(lib, lg.contiguous(), w[0], w[1], w[2], seed=m.seed, n=n)
    print(f"{side.name}: ids behind the fork {ids.tolist()}, the op's with (seed {m.seed}, row r, n {n}) {want.tolist()}, u {info[:, 3].tolist()}")
    assert ids.tolist() == want.tolist()
    assert len(set(info[:, 3].tolist())) == 3                    # three streams ...
    row0 = [int(L.sample(lib, lg[r:r + 1].contiguous(), w[0], w[1], w[2], seed=m.seed, n=n)[0][0]) for r in range(3)]
    assert row0 != want.tolist()                                 # ... that row 0's stream alone would not have given (a property of the seed)
    other = L.sample(lib, lg.contiguous(), w[0], w[1], w[2], seed=m.seed, n=n - 1)[0]
    assert other.tolist() != want.tolist()                       # and a host-side step count (one short of the moved length) neither


@pytest.mark.parametrize("fmt", ["bf16", "e4m3", "mxfp4"])
def test_k_the_draw_under_moved_state(fmt):
    side, _ = _sides("k", fmt)
    S.script_k(side, seed=_seed("k", fmt), draw_check=_draw_check)


# ---- l: log-probability provenance ----------------------------------------------------------------------------------------------------------------
def _lp(side, logits, ids, passed):
    """fvhd_llm_logprobs(ctx, passed or NULL, n) for n in {0, 5, 16} against the fp64 reference on `logits` under its derived bound"""
    gen, B, dev = side.gen, side.gen._run_batch, side.gen.device
    ref = LR.Reference(logits, ids, 16)
    worst = 0.0
    for n in (0, 5, 16):
        tok = torch.full((B,), float("nan"), device=dev)
        top_ids = torch.full((B, n), -7, device=dev, dtype=torch.long) if n else None
        top_lp = torch.full((B, n), float("nan"), device=dev) if n else None
        gen.logprobs(n, tok, top_ids, top_lp, logits=passed)
        torch.cuda.synchronize()
        worst = max(worst, ref.check(n, tok, top_ids, top_lp, what=f"{side.name} n={n}"))
    print(f"{side.name}: logprobs({'the passed buffer' if passed is not None else 'NULL'}) at length {side.model.length}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("proc", [False, True], ids=["plain", "processors"])
def test_l_logprob_provenance(proc):
    key = "lp" if proc else "l"
    side, twin = _sides(key)
    S.script_l(side, twin, seed=_seed(key), lp=_lp, proc=proc)


# ---- m: a captured graph keeps its settings -------------------------------------------------------------------------------------------------------
def _capture(dev, body):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            body()
    torch.cuda.current_stream(dev).wait_stream(s)
    return g


def test_m_a_captured_step_keeps_its_processors_and_seed():
    """one step captured under (processors X, seed s); then (Y, t) are set; the replay equals the twin's eager step under (X, s) bit for
    bit, the eager step enqueued afterwards the twin's under (Y, t)"""
    side, twin = _sides("m")
    gen, dev = side.gen, side.gen.device
    e, mask, fed1, r1, fed2, r2 = S.script_m(twin, seed=_seed("m"))
    side.set_processors(**S.PROC_J)
    side.set_sampling(True, seed=S.M_S, **S.SAMPLING)
    side.start(e, mask, what="m start")
    fed = torch.tensor(fed1, device=dev)
    lg_out, ids_out = torch.empty_like(gen._logits[:S.M_B]), torch.empty_like(gen._ids[:S.M_B])

    def body():
        lg, ids = gen.step(fed)
        lg_out.copy_(lg)
        ids_out.copy_(ids)

    g = _capture(dev, body)
    assert gen.cache_state() == (S.M_P, 0)                       # capturing enqueued nothing
    gen._length = S.M_P
    # the library gets (Y, t) now; the model after the replay: the settings are an enqueue-time matter - the captured step is X's and s's
    side._set_processors(S.PROC_Y)
    side._set_sampling(True, S.M_T, *side.warp)
    g.replay()
    torch.cuda.synchronize()
    gen._length = S.M_P + 1
    lg, ids = side.step(fed1, what="m replay under (Y, t) of a step captured under (X, s)", got=(lg_out, ids_out))
    assert side.model.drawn == [(r, S.M_P + 1) for r in range(S.M_B)]
    side.same(lg, r1[0], "the replay equals the eager step under (X, s)")
    assert ids.tolist() == r1[1].tolist()
    side.model.set_processors(**S.PROC_Y)
    side.model.set_sampling(True, S.M_T)
    lg, ids = side.step(fed2, what="m eager step behind the replay")
    side.same(lg, r2[0], "the eager step behind the replay follows (Y, t)")
    assert ids.tolist() == r2[1].tolist()
    # the two settings tell the steps apart: the scores of X are not those of Y on the same raw logits
    assert not L.same_bits(r1[0], r2[0])


def test_m_a_captured_step_keeps_leaving_its_logits():
    """set_logprobs(1), one greedy step without a logits_out captured, set_logprobs(0), replay: the step still left its logits in the
    context's buffer - the numbers fvhd_llm_logprobs(NULL) gives once the setting is on again are those of the twin's eager step"""
    side, twin = _sides("m")
    gen, dev = side.gen, side.gen.device
    e, mask = S.rows(side.ref, S.M_B, S.M_P, _seed("m"))
    tlg, tids = twin.start(e, mask, what="m start (twin)")
    fed1 = tids.tolist()
    t1 = twin.step(fed1, what="m eager step (twin)")
    side.set_logprobs(True)
    _, ids = side.start(e, mask, what="m start", given=False, raw=tlg)
    _lp(side, tlg, ids, None)
    fed = torch.tensor(fed1, device=dev)
    g = _capture(dev, lambda: gen.step(fed, logits=False))
    gen._length = S.M_P
    side.set_logprobs(False)
    g.replay()
    torch.cuda.synchronize()
    gen._length = S.M_P + 1
    side.model.set_logprobs(True)                                # the step was enqueued (captured) with the setting on
    side.step(fed1, what="m replay with the setting switched off since", got=(None, gen._ids[:S.M_B]), given=False, raw=t1[0])
    side.model.set_logprobs(False)
    side.refused(CM.LP_OFF, lambda m: m.logprobs(), lambda g_: g_.logprobs(0, torch.zeros(S.M_B, device=dev)))
    side.set_logprobs(True)
    assert side.model.logprobs() and gen._ids[:S.M_B].tolist() == t1[1].tolist()
    _lp(side, t1[0], t1[1], None)
    side.set_logprobs(False)


# ---- the pair sweep ---------------------------------------------------------------------------------------------------------------------------------
OPS = ["start", "step_none", "step_ids", "extend", "rewind", "gather", "verify", "lookup", "score_last", "logprobs_null"]
SETTINGS = ["plain", "sampling", "processors", "logprobs"]
SWEEP_P, SWEEP_T, SWEEP_CAP, SWEEP_NEW = 9, 3, 48, 8
REASONS = [CM.NO_CHUNK_IDS, CM.NOT_REWOUND, CM.NOT_REORDERED, CM.NOT_MAINTAINED, CM.GREEDY_ONLY, CM.NO_HISTORY, CM.LP_OFF, CM.LP_NOT_LAST, CM.LP_NO_SCRATCH,
           "before the cache reorder / rewind", "ONE sequence", "no token buffer"]
COUNTS = {}


def _reason(err):
    """the reason a refusal names: the first of REASONS in its words (else the words themselves, which then equal nothing of the model's)"""
    return next((r for r in REASONS if r in str(err)), str(err))


@functools.lru_cache(maxsize=None)
def _sweep_context(setting):
    """one context per setting (a generator owns its context's cache), reused across the pairs; every allocation a call may grow - the
    chunk workspace at B = 2, the scratches - made before the first pair, under no setting"""
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, ref, _ = _contexts("bf16")
    gen = Qwen2Generator.from_hf(m16, 2, SWEEP_CAP, prefill=Qwen2Prefill.from_hf(m16))
    gen.spec_reserve(16, 64)
    gen.beam_reserve()
    H = ref.config.hidden_size
    gen.start(torch.zeros(1, SWEEP_P, H, device=gen.device, dtype=torch.bfloat16))
    gen.cache_gather(torch.zeros(2, device=gen.device, dtype=torch.long), 1)
    gen.extend(torch.zeros(2, SWEEP_T, H, device=gen.device, dtype=torch.bfloat16))
    gen.set_sampling(setting == "sampling", seed=5, **S.SAMPLING)
    gen.set_logits_processors(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[3, 9]) if setting == "processors" else gen.set_logits_processors()
    gen.set_logprobs(setting == "logprobs")
    model = CacheModel(2, SWEEP_CAP, ref.get_input_embeddings().weight)
    model.set_sampling(setting == "sampling", 5)
    if setting == "processors":
        model.set_processors(**S.PROC_J)
    model.set_logprobs(setting == "logprobs")
    g = torch.Generator().manual_seed(3)
    data = dict(e=(0.5 * torch.randn(1, SWEEP_P, H, generator=g)).to(torch.bfloat16), c=(0.5 * torch.randn(2, SWEEP_T, H, generator=g)).to(torch.bfloat16),
                out=torch.zeros(SWEEP_NEW, device=gen.device, dtype=torch.long), lib=_lib.lookup_lib(), eos=(C.c_int32 * 1)(0))
    return gen, model, data


def _run_op(op, gen, model, data, given, level):
    """one call on the library and on the model -> ((ran | refused, reason) of the library, of the model)"""
    from ml_fastvlm_amd import _lib
    dev, B = gen.device, model.run_batch
    procs = gen._processors
    if level == "library":                                      # past the generator's own refusals: the library's are the ones asked
        gen._processors, gen._ids_stale, gen._do_sample = None, False, False
    got = want = ("ran", None)
    ids = None
    try:
        if op == "start":
            _, ids = gen.start(data["e"].to(dev), None, logits=given)
        elif op == "step_none":
            _, ids = gen.step(None, logits=given)
        elif op == "step_ids":
            _, ids = gen.step(torch.arange(20, 20 + B, device=dev), logits=given)
        elif op == "extend":
            _, ids = gen.extend(data["c"][:B].to(dev), None, logits=given)
        elif op == "rewind":
            gen.rewind([model.length - 1] * B)
        elif op == "gather":
            gen.cache_gather(torch.zeros(2, device=dev, dtype=torch.long), B)
        elif op == "verify":
            _, ids, emitted = gen.verify(torch.tensor([1, 2, 3], device=dev))
        elif op == "lookup":
            lib, h, st = data["lib"], gen.pre._h, _lib.stream_ptr(dev)
            _lib.check(lib.fvhd_llm_lookup_begin(h, None, 0, C.cast(data["eos"], C.c_void_p), 0, SWEEP_NEW, _lib.ptr(data["out"]), st), "fvhd_llm_lookup_begin")
            _lib.check(lib.fvhd_llm_lookup_step(h, 4, 2, st), "fvhd_llm_lookup_step")
            gen._length = None
            written = gen.lookup_state()[0]
            ids = (data["out"][1:written].tolist() + [-1] * 4)[:4]
        elif op == "score_last":
            lab = torch.zeros(model.last_chunk, device=dev, dtype=torch.long)
            assert tuple(gen.score_last(lab)[0].shape) == model.last_chunk
        elif op == "logprobs_null":
            gen.logprobs(0, torch.zeros(B, device=dev))
    except (ValueError, RuntimeError) as err:                   # (FvhdError is a RuntimeError)
        got = ("refused", _reason(err))
    finally:
        gen._processors = procs
    back = [0] * 2 if ids is None else (ids.tolist() if isinstance(ids, torch.Tensor) else ids)
    try:
        if op == "start":
            assert model.start(data["e"].float(), None, back[:1], logits_given=given)
        elif op == "step_none":
            assert model.step(None, back[:B], logits_given=given)
        elif op == "step_ids":
            assert model.step(list(range(20, 20 + B)), back[:B], logits_given=given)
        elif op == "extend":
            assert model.extend(data["c"][:B].float(), None, back[:B], logits_given=given)
        elif op == "rewind":
            assert model.rewind([model.length - 1] * B)
        elif op == "gather":
            assert model.gather([0, 0], B)
        elif op == "verify":
            assert model.verify([1, 2, 3], back[:4]) >= 1
        elif op == "lookup":
            model.lookup_begin(None, [], SWEEP_NEW)
            assert model.lookup_step(4, 2, back[:4]) >= 1
        elif op == "score_last":
            assert model.score_last() is not None
        elif op == "logprobs_null":
            assert model.logprobs()
    except Refused as err:
        want = ("refused", _reason(err))
    if level == "library":                                      # the generator's own flags again, as the model has them
        gen._ids_stale, gen._do_sample = model.ids_stale, model.sampling
    return got, want


@pytest.mark.parametrize("first", OPS)
@pytest.mark.parametrize("level", ["generator", "library"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_pair_sweep(setting, level, first):
    """start -> `first` -> every second call, under one setting: after each call the library's outcome equals the model's; `level`: through
    the generator as it is, or with the generator's own refusals out of the way (the library's are then the ones that answer)"""
    gen, model, data = _sweep_context(setting)
    given = setting != "logprobs"                                # under the log-probability setting the calls keep their logits
    ran = refused = 0
    for second in OPS:
        got, want = _run_op("start", gen, model, data, given, level)
        assert got == want == ("ran", None)
        # a fresh start resets everything the sweep looks at
        assert (model.run_batch, model.state(), model.ids_stale, model.lookup, model.hist[0]) == (1, (SWEEP_P, 0), False, None, [])
        assert model.hist_started == (setting == "processors") and model.lp_where == (None if given else "start")
        for i, op in enumerate((first, second, "step_none")):    # the closing step(None): whether it is still allowed
            if i == 2:
                model_allowed = model.may_step_none()            # (asked before the call: the model's own answer, not its step's)
            got, want = _run_op(op, gen, model, data, given, level)
            what = (setting, level, first, second, i, op)
            assert got == want, (what, got, want)
            assert gen.length() == model.length and gen.cache_state() == model.state() and gen._run_batch == model.run_batch, \
                (what, gen.length(), gen.cache_state(), gen._run_batch, model.state(), model.run_batch)
            if i < 2:
                ran, refused = ran + (got[0] == "ran"), refused + (got[0] == "refused")
        assert (got[0] == "ran") == model_allowed, (setting, level, first, second, got, model_allowed)
    c = COUNTS.setdefault((setting, level), [0, 0])
    c[0], c[1] = c[0] + ran, c[1] + refused
    print(f"sweep {setting} / {level}: first = {first}: {ran} calls ran, {refused} refused; so far under this setting {c[0]} ran, {c[1]} refused")
