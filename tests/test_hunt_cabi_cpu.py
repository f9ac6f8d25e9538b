"""The hunt environment's C entry points on a host without a GPU: the range marl_hunt_supported states, every refusal of the four
launchers (made before anything is dereferenced or launched: the pointers here are widths-only placeholders, no device memory is
touched), and the shape of their signatures."""
import ctypes as C

import pytest

INVALID = 1                                           # hipErrorInvalidValue
ENTRIES = {"marl_hunt_reset": ("units",), "marl_hunt_step": ("act", "units", "alive_next"),
           "marl_hunt_fused_step": ("q", "units"), "marl_hunt_fused_step_sample": ("q", "units")}
E, T, N, M, G, A, O = 3, 5, 4, 2, 8, 6, 77
S = 2 * N + 3 * M
PTR = C.c_void_p(4096)                                # never dereferenced: every call below is refused first


def _record(**kw):
    from marl_amd import _lib
    f = dict(state_ld=S, E=E, T=T, N=N, O=O, S=S, A=A)
    f.update(kw)
    return C.byref(_lib.MarlRecord(obs=4096, state=4096, avail=4096, u=4096, r=4096, term=4096, padded=4096, length=4096, won=4096,
                                   **f))


def _calls(rec, M=M, G=G, pen4=8, t=0, reset=True):
    """the return codes of the four launchers; reset = False: of the three that take pen4 and t (reset would not refuse)"""
    from marl_amd import _lib
    lib = _lib.load()
    return ([lib.marl_hunt_reset(1, 0, 0, G, M, PTR, rec, None)] if reset else []) + [
            lib.marl_hunt_step(1, 0, 0, G, pen4, t, PTR, PTR, rec, PTR, M, None),
            lib.marl_hunt_fused_step(1, 2, 0, 0, G, pen4, t, 0.5, PTR, PTR, rec, M, None),
            lib.marl_hunt_fused_step_sample(1, 2, 0, 0, G, pen4, t, 0.5, PTR, PTR, rec, M, None)]


def test_supported_range():
    from marl_amd import ops
    ok = ops.hunt_supported
    assert ok(2, 1, 3, 6) and ok(16, 16, 32, 6) and ok(4, 2, 8, 6) and ok(2, 16, 32, 6) and ok(16, 1, 3, 6)
    assert not ok(1, 1, 6, 6) and not ok(17, 1, 6, 6)            # predators: 2 .. 16
    assert not ok(2, 0, 6, 6) and not ok(2, 17, 6, 6)            # prey: 1 .. 16
    assert not ok(2, 1, 2, 6) and not ok(2, 1, 33, 6)            # grid side: 3 .. 32
    assert not ok(2, 1, 6, 5) and not ok(2, 1, 6, 7)             # six actions


def test_every_entry_refuses_what_the_header_lists():
    assert _calls(None) == [INVALID] * 4                                             # no record
    assert _calls(_record(O=O + 1)) == [INVALID] * 4                                 # widths other than the derived ones
    assert _calls(_record(S=S + 1, state_ld=S + 4)) == [INVALID] * 4
    assert _calls(_record(S=S - 1)) == [INVALID] * 4
    assert _calls(_record(state_ld=S - 1)) == [INVALID] * 4                          # a state row stride below S
    assert _calls(_record(T=0)) == [INVALID] * 4
    for t in (-1, T, T + 1):                                                         # a step outside the episode
        assert _calls(_record(), t=t, reset=False) == [INVALID] * 3
    for n, m, g, a in ((1, 2, 8, 6), (17, 2, 8, 6), (4, 0, 8, 6), (4, 17, 8, 6), (4, 2, 2, 6), (4, 2, 33, 6), (4, 2, 8, 7)):
        rec = _record(N=n, A=a, S=2 * n + 3 * m, state_ld=2 * n + 3 * m + 4)
        assert _calls(rec, M=m, G=g) == [INVALID] * 4, (n, m, g, a)                  # what marl_hunt_supported refuses
    for pen4 in (-1, 65, 1 << 20):                                                   # the penalty's range
        assert _calls(_record(), pen4=pen4, reset=False) == [INVALID] * 3


def test_an_empty_batch_launches_nothing():
    assert _calls(_record(E=0)) == [0] * 4 and _calls(_record(E=-3)) == [0] * 4      # (after the shape checks: they passed)


def test_signatures_one_record_and_the_stream_last():
    from marl_amd import _lib
    P, I = _lib.P, _lib.I
    rec = C.POINTER(_lib.STRUCTS["marl_record_t"])
    for name, loose in ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is I and args.count(rec) == 1, name
        assert args[-1] is P and args[:-1].count(P) == len(loose), (name, "loose pointers beside the record (and the stream)")
    assert _lib.SIGNATURES["marl_hunt_supported"] == (I, [I, I, I, I])
    with pytest.raises(AttributeError):
        _lib.load().marl_hunt_rollout                                                # no whole-rollout entry: out of scope
