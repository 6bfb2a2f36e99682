"""The soak's control: can tests/soak.py see a broken hand-off on THIS machine?

tests/soak_control.hip's k_ticket_sum is the ticket reducer of k_tree_group_f32_norm's end (norm_finish)
in miniature: G workgroups store a partial each, pre-read the partial lines (an L1-warm consumer), take a
ticket, and the last arriver reads all partials and writes how many differ from the input to out[0].
MODE 0 is the product's form (write-through store, vmcnt(0), relaxed agent ticket, one lane's agent
acquire, barrier, plain loads); MODE 1 has plain stores, no release and no acquire.

Both run through soak() — one capture, R replays back to back, `in` alternating between two random
images that differ in every word, so a partial left from the replay before is a wrong value — under
each load.  MODE 0 must show 0 stale reads in R replays.  MODE 1 must show at least one: without that
a green soak of the product's kernels would prove nothing here.  The stale fractions observed on an
MI355X are in profiles/soak_control.json and DESIGN.md.

Buffers: in (restored every replay, only read), partials (never restored; after a launch they equal
`in`, whole), the counter (zeroed once; 0 after every launch), out (restored to 0xFFFFFFFF every replay,
so a launch that does not write it fails)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import soak  # noqa: E402  (needs torch)

pytestmark = pytest.mark.gpu
G = 256   # workgroups: 1 KiB of partials, eight 128-byte lines, spread over every XCD
OUT = 3   # the index of `out` in the case's buffers


def ticket_case(kernel_mode):
    rng = np.random.default_rng(17)
    a = rng.integers(0, 1 << 32, G, dtype=np.uint64).astype(np.uint32)
    b = a ^ rng.integers(1, 1 << 32, G, dtype=np.uint64).astype(np.uint32)   # differs from a in every word
    assert (a != b).all()
    dev = {name: torch.zeros(n, dtype=torch.int32, device=soak.DEV) for name, n in (("in", G), ("partials", G), ("counter", 16), ("out", 16))}
    zero, ones = np.zeros(16, dtype=np.uint32), np.full(16, 0xFFFFFFFF, dtype=np.uint32)
    after = ones.copy()
    after[0] = 0
    bufs = [soak.SoakBuf("in", dev["in"], [a, b], [a, b]),
            soak.SoakBuf("partials", dev["partials"], None, [a, b]),
            soak.SoakBuf("counter", dev["counter"], None, [zero, zero]),
            soak.SoakBuf("out", dev["out"], [ones, ones], [after, after])]
    assert bufs[OUT].name == "out"

    def call(s):
        rc = soak.control().ticket_sum(kernel_mode, dev["in"].data_ptr(), dev["partials"].data_ptr(), dev["counter"].data_ptr(),
                                       dev["out"].data_ptr(), G, s.cuda_stream)
        assert rc == 0, f"ticket_sum returned {rc}"
    return soak.Case(bufs, call)


@pytest.mark.parametrize("mode", soak.MODES)
def test_the_products_form_is_never_stale(mode):
    bad, _, report = soak.soak(ticket_case(0), soak.R, mode)
    assert not bad.any()
    print(f"control MODE 0 under {mode}: 0 stale replays of {soak.R}; one load launch {report['load_launch_ms']} ms")


@pytest.mark.parametrize("mode", soak.MODES)
def test_the_broken_form_is_seen(mode):
    bad, _, _ = soak.soak(ticket_case(1), soak.R, mode, expect_clean=False)
    stale = int((bad[:, OUT] != 0).sum())
    print(f"control MODE 1 under {mode}: {stale} stale replays of {soak.R} ({stale / soak.R:.3f}); "
          f"differing elements per buffer: {bad.sum(axis=0).tolist()}")
    assert not bad[:, 0].any(), "`in` is only read"
    assert stale >= 1, "the soak cannot see a hand-off without release and acquire on this machine: a green soak proves nothing"
