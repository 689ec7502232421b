"""Every operator held to its launch contract: "launched on `stream`, no host synchronisation, no allocation
(graph-capturable)" — what bench.py measures through when it replays a captured graph.

For every row of tests/capture_cases.py (every operator function and C entry of the alignment registry, and the module-level
rows production captures), on the GPU:

  a. host-read probe    the call under torch's sync debug mode "error".  A row of HOST_READS must raise there (so the
                        exclusion cannot go stale) and is never captured; every other row must pass.
  b. side stream        work is queued on a fresh stream in front of the call and one operand is written behind that work;
                        the call, made on that stream, must give the eager result.  A launch on another stream reads the
                        operand before it is written.
  c. decoy capture      the eager result on the true operands is the yardstick.  Every floating operand is zeroed, the call
                        is recorded with torch.cuda.graph on a side stream, the true contents are copied back, every output
                        is filled with a sentinel, the graph is replayed: outputs and in-place operands must have the eager
                        bits (rows with float atomics: within the bound their parity test uses), twice.  A launch on
                        another stream, a launch left out of the graph, a value baked in at capture and an output not
                        written on replay all show as different bits.
  d. cold capture       rows that own a packed-weight cache: a fresh wrapper's first call ever is recorded; before any
                        replay an eager call must have the reference's bits, then the replay, then an eager call after an
                        in-place weight change the bits for the new weights.

After an error during capture or replay that is not an argument refusal, nothing more is started on the device.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import alignment_cases as AC       # noqa: E402  (it needs torch at import)
from tests import capture_cases as CC         # noqa: E402

_STOP = []     # set after an unexpected error during capture or replay: the remaining GPU tests skip
SENTINEL = 77


# ---- the harness (torch only) ------------------------------------------------------------------------------------------
def tensors_of(a):
    return {k: v for k, v in a.items() if isinstance(v, torch.Tensor)}


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


def restore(a, truth, keys=None):
    for k in (truth if keys is None else keys):
        a[k].copy_(truth[k])


def host_read_probe(call, a):
    """None and the outputs if the call reads nothing on the host, else the message of torch's sync debug mode."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return None, call(a)
    except RuntimeError as exc:
        if "synchronizing" not in str(exc):
            raise
        return str(exc), None
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def gate_key(a, inplace):
    """The operand the side-stream test writes late: the first floating one the call does not write, else the first of any type."""
    ts = {k: v for k, v in tensors_of(a).items() if k not in inplace and v.numel()}
    floats = [k for k, v in ts.items() if v.is_floating_point()]
    return (floats or list(ts))[0]


def on_a_side_stream(call, a, truth, inplace):
    key = gate_key(a, inplace)
    a[key].zero_()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s), torch.no_grad():
        torch.randn(1 << 22, device=a[key].device).sort()      # work queued on s in front of the call ...
        a[key].copy_(truth[key])                                # ... and the operand exists only once s has got there
        outs = call(a)
    s.synchronize()
    torch.cuda.synchronize()
    return outs


def _guarded(what, fn, refusals=()):
    try:
        return fn()
    except refusals:
        raise
    except Exception as exc:
        if "(code 100001)" not in str(exc):      # LGU_E_BADARG through _lib.check is an argument refusal
            _STOP.append("%s: %s: %s" % (what, type(exc).__name__, exc))
        raise


def capture_on_decoys_replay_on_truth(call, a, truth, inplace, check, refusals=()):
    """Step c.  check(outs, what) compares a call's outputs and the in-place operands with the yardstick."""
    for k, v in tensors_of(a).items():
        if v.is_floating_point():
            v.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def record():
        with torch.cuda.graph(g, stream=s):
            return call(a)
    outs = _guarded("capture", record, refusals)
    torch.cuda.synchronize()
    args_at = {v.data_ptr() for v in tensors_of(a).values()}
    for what in ("first replay", "second replay"):
        restore(a, truth)
        for o in outs:
            if o is not None and o.data_ptr() not in args_at:
                o.fill_(SENTINEL)
        torch.cuda.synchronize()
        _guarded(what, lambda: (g.replay(), torch.cuda.synchronize()))
        check(outs, what)
    return g


def run_row(call, a, inplace, host_reads, captured, check_factory):
    """Steps a to c for one row; returns what was done.  check_factory(yardstick outputs, in-place results) -> check."""
    truth = {k: v.clone() for k, v in tensors_of(a).items()}
    if host_reads:
        call(a)                                  # warm: what only a first call uploads or initialises is not the finding
        restore(a, truth)
        msg, _ = host_read_probe(call, a)
        assert msg is not None, "listed as reading the host, but the call synchronises nowhere"
        return "host read: " + msg.splitlines()[0]
    outs0 = call(a)
    torch.cuda.synchronize()
    yard = [None if o is None else o.clone() for o in outs0]
    yard_inplace = {k: a[k].clone() for k in inplace}
    check = check_factory(yard, yard_inplace, a)
    restore(a, truth)
    msg, outs = host_read_probe(call, a)
    assert msg is None, "the call reads the host: " + msg.splitlines()[0]
    check(outs, "under the sync debug mode")
    restore(a, truth)
    check(on_a_side_stream(call, a, truth, inplace), "on a side stream")
    if not captured:
        return "probe and side stream"
    restore(a, truth)
    capture_on_decoys_replay_on_truth(call, a, truth, inplace, check)
    return "captured"


def bitwise(yard, yard_inplace, a):
    def check(outs, what):
        assert len(outs) == len(yard), what
        for i, (g, w) in enumerate(zip(outs, yard)):
            assert (g is None) == (w is None) and (g is None or same_bits(g, w)), "%s: output %d differs from the eager call" % (what, i)
        for k, w in yard_inplace.items():
            assert same_bits(a[k], w), "%s: in-place operand %s differs from the eager call" % (what, k)
    return check


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_every_stream_entry_is_captured_or_placed_with_a_reason():
    entries = CC.stream_entries()
    assert len(entries) == len(set(entries)) == 99, len(entries)
    names = [c.name for c in CC.ROWS]
    assert len(names) == len(set(names))
    assert set(CC.HOST_READS) <= set(names) and set(CC.NOT_CAPTURED) <= set(names) and set(CC.COLD) <= set(names)
    assert not set(CC.HOST_READS) & set(CC.NOT_CAPTURED)
    assert not set(CC.COLD) & (set(CC.HOST_READS) | set(CC.NOT_CAPTURED))
    captured = {s for c in CC.captured_rows() for s in c.symbols}
    host = {s for c in CC.ROWS if c.name in CC.HOST_READS for s in c.symbols} - captured
    left = {s for c in CC.ROWS if c.name in CC.NOT_CAPTURED for s in c.symbols} - captured - host
    assert captured | host | left <= set(entries), sorted((captured | host | left) - set(entries))
    missing = sorted(set(entries) - captured - host - left)
    assert not missing, "no capture row and no stated exclusion for: %s" % ", ".join(missing)
    for table in (CC.HOST_READS, CC.NOT_CAPTURED):
        assert all(len(r.strip()) > 10 and "\n" not in r for r in table.values())
    print("%d stream entries: %d captured, %d behind a host read only, %d not captured" % (len(entries), len(captured), len(host), len(left)))
    assert not left      # today nothing is left to NOT_CAPTURED alone: the two-launch norm's entry is captured on its single-launch path
    # what the header itself calls graph-capturable is captured, through ctypes where the Python operator reads the host
    claimed = ["lgu_projective_transform_f32", "lgu_motion_features_f32", "lgu_scatter_mean_f32", "lgu_scatter_mean_h16", "lgu_cvx_upsample_f32",
               "lgu_upsample_disps_f32", "lgu_proximity_select_small", "lgu_proximity_keys", "lgu_proximity_select_sorted",
               "lgu_instnorm_relu_f32", "lgu_instnorm_relu_h16", "lgu_cloud_decide_f32", "lgu_cloud_write_f32"]
    claimed += ["lgu_%s_%s" % (k, t) for k in ("kangru_context", "kan_heads", "kangru_gates", "kangru_blend") for t in ("f32", "h16")]
    assert set(claimed) <= captured, sorted(set(claimed) - captured)
    # only the BA's kernels stay behind a host read: ba.ba builds its plan from the edge set on the host
    assert all(s.startswith("lgu_ba_") for s in host), sorted(host)


def test_the_struct_argument_entries_have_rows_in_both_audits():
    from tests.test_alignment import STRUCT_ARGS
    captured = {s for c in CC.captured_rows() for s in c.symbols}
    aligned = {s for c in AC.CASES for s in c.symbols}
    assert set(STRUCT_ARGS) <= captured and set(STRUCT_ARGS) <= aligned


def test_design_table_places_every_entry_and_row():
    """DESIGN.md section 4.3 names every stream entry and every row that is not captured, with its reason."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md")).read()
    m = re.search(r"^### 4\.3 .*?(?=^## 5\. )", text, flags=re.S | re.M)
    assert m, "DESIGN.md has no section 4.3"
    body = m.group(0)
    named = set(re.findall(r"lgu_[a-z0-9_]+", body))
    assert set(CC.stream_entries()) <= named, sorted(set(CC.stream_entries()) - named)
    for name in list(CC.HOST_READS) + list(CC.NOT_CAPTURED) + list(CC.COLD) + [c.name for c in CC.EXTRA]:
        assert "`%s`" % name in body, "section 4.3 does not name the row %s" % name


def test_a_pack_made_while_capturing_is_used_and_not_kept(lgu, monkeypatch):
    H = lgu._host
    w = torch.zeros(3)
    made = []

    def make():
        made.append(object())
        return made[-1]
    cache = H.PackCache()
    monkeypatch.setattr(H, "capturing", lambda device=None: True)
    first, second = cache.get("slot", [w], make), cache.get("slot", [w], make)
    assert first is made[0] and second is made[1] and cache._slots == {}
    monkeypatch.setattr(H, "capturing", lambda device=None: False)
    kept = cache.get("slot", [w], make)
    assert kept is made[2] and cache.get("slot", [w], make) is kept and len(made) == 3 and len(cache._slots) == 1
    monkeypatch.setattr(H, "capturing", lambda device=None: True)      # a hit stored before the capture is used as it is
    assert cache.get("slot", [w], make) is kept and len(made) == 3
    w.add_(1)                                                           # ... and a miss under capture leaves the old entry alone
    assert cache.get("slot", [w], make) is made[3] and cache._slots["slot"][1] is kept


def test_the_predicate_is_false_without_a_capture(lgu):
    assert lgu._host.capturing() is False
    lgu._host.no_upload_while_capturing("nothing")


# ---- GPU: the harness can fail ---------------------------------------------------------------------------------------------
def _need_gpu(lgu=None):
    if _STOP:
        pytest.skip("an earlier capture or replay ended in an error, nothing more is started on the device: %s" % _STOP[0])
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if lgu is not None:
        assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


@pytest.mark.gpu
def test_the_harness_passes_a_sound_row_and_fails_the_two_defects():
    """Torch operations only, never the library: x * 2 passes; a toy that returns what it computed at its first call fails
    step c (a value baked in); a toy that calls float(x.sum()) is classified as a host read by step a."""
    _need_gpu()

    def fresh():
        return dict(x=torch.randn(257, generator=torch.Generator().manual_seed(1)).cuda())
    assert run_row(lambda a: (a["x"] * 2,), fresh(), (), False, True, bitwise) == "captured"

    def baked(a, kept=[]):
        if not kept:
            kept.append(a["x"] * 2)                            # the result, computed at the first call and handed out ever after
        a["x"] + 1                                             # (some launch, so that the recorded graph is not empty)
        return (kept[0],)
    with pytest.raises(AssertionError, match="first replay: output 0 differs"):
        run_row(baked, fresh(), (), False, True, bitwise)
    assert not _STOP

    def reads_host(a):
        return (a["x"] * float(a["x"].sum()),)
    with pytest.raises(AssertionError, match="the call reads the host"):
        run_row(reads_host, fresh(), (), False, True, bitwise)
    assert run_row(reads_host, fresh(), (), True, False, bitwise).startswith("host read")
    with pytest.raises(AssertionError, match="synchronises nowhere"):
        run_row(lambda a: (a["x"] * 2,), fresh(), (), True, False, bitwise)

    def wrong_stream(a):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return (a["x"] * 2,)
    with pytest.raises(AssertionError, match="on a side stream: output 0 differs"):
        run_row(wrong_stream, fresh(), (), False, True, bitwise)
    assert not _STOP


# ---- GPU: every row ------------------------------------------------------------------------------------------------------
_REF = {}


def _check_factory(lgu, oracle, c, host_args):
    atomics = c.bound is not None and c.bound[1] is AC.REL_1E5      # float atomics: not bit-reproducible, held to the oracle
    if not atomics:
        return bitwise

    def factory(yard, yard_inplace, a):
        ref_fn, tol = c.bound
        if c.name not in _REF:
            _REF[c.name] = ref_fn(oracle, host_args)

        def check(outs, what):
            for i, (g, w) in enumerate(zip(outs, _REF[c.name])):
                err = float(np.abs(g.detach().cpu().numpy().reshape(w.shape) - w).max())
                print("%s %s output %d: max abs err %.3g (bound %.3g)" % (c.name, what, i, err, tol(w)))
                assert err <= tol(w), (c.name, what, i, err, tol(w))
            for k, w in yard_inplace.items():
                assert same_bits(a[k], w), "%s: in-place operand %s differs from the eager call" % (what, k)
        return check
    return factory


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CC.ROWS])
def test_row_keeps_its_launch_contract(lgu, oracle, name):
    _need_gpu(lgu)
    c = CC.BY_NAME[name]
    a = c.build(torch.device("cuda:0"))
    host_args = {k: v.detach().cpu().numpy() for k, v in tensors_of(a).items() if v.dtype != torch.float16} if c.bound else None
    done = run_row(lambda args: c.call(lgu, args), a, c.inplace, name in CC.HOST_READS, name not in CC.NOT_CAPTURED,
                   _check_factory(lgu, oracle, c, host_args))
    print("%s: %s" % (name, done))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CC.COLD))
def test_first_call_ever_under_capture_leaves_no_unwritten_pack_behind(lgu, name):
    """Step d.  A PackCache.get that keeps what `make()` returned while the stream was only recording (the parent's) fails
    the first comparison of every row that owns a PackCache: the eager call behind the capture hits the cache and reads a
    pack that no kernel has written yet."""
    _need_gpu(lgu)
    a, run, want, change = CC.COLD[name](lgu, torch.device("cuda:0"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def record():
        with torch.cuda.graph(g, stream=s):
            return run()
    cap = _guarded("cold capture", record)
    torch.cuda.synchronize()
    ref = want()                                        # the same layers under a wrapper that never saw a capture
    got = run()                                         # eager, before any replay
    torch.cuda.synchronize()
    assert len(got) == len(ref) == len(cap) > 0
    assert all(same_bits(x, y) for x, y in zip(got, ref)), "the eager call behind a cold capture differs from the reference"
    _guarded("replay", lambda: (g.replay(), torch.cuda.synchronize()))
    assert all(same_bits(x, y) for x, y in zip(cap, ref)), "the replay of a cold capture differs from the reference"
    if change is not None:
        change()
        got2, ref2 = run(), want()
        torch.cuda.synchronize()
        assert len(got2) == len(ref2) == len(got)
        assert all(same_bits(x, y) for x, y in zip(got2, ref2)), "after an in-place weight change the eager call is not the new weights'"
        assert not all(same_bits(x, y) for x, y in zip(got2, got)), "the weight change changed nothing: the test shows nothing"
