"""Every kernel route of the one-GPU engine (tests/route_cases.py) on hard inputs.

Per case and dataset (tests/hard_inputs.py: `cancel`, whose result depends on the order of the
adds, and `nonfinite`):
  1. every buffer the call may touch is filled with a sentinel and compared WHOLE: the rank rows at
     preferred_rank_stride with a guard row in front of row 0, the stride skew and a guard row
     behind the last rank; the workspace between two 256-byte guards; out / in / shard buffers
     with a gap behind every row and guard rows.  The expected image is the CPU oracle where the
     operation defines a result, the input bits where it only reads (a fused reduce-scatter in
     place keeps every block it does not own), the sentinel everywhere else;
  2. cancel: 0 differing elements, bit for bit.  nonfinite: bit-exact outside the planted columns;
     inside them NaN as a class, +Inf / -Inf as bits, on every rank that receives the column — held
     against the oracle AND against the answer hard_inputs states;
  3. the launch trace of the call is the case's expected list of kernel names, and its count is
     plan.launches (the grouped calls: the dry launch count) under the same tune keys.
The schedule-form MEM plan's workspace holds the reduced vector; its content is compared too.
The buffers, expected images and calls are those of tests/route_run.py, shared with the side-stream
and far-stride modules; this one runs them on the default stream.
"""
import pytest

import route_cases
import tenstorrentallreduce_amd as t

torch = pytest.importorskip("torch")
import route_run  # noqa: E402  (needs torch)

pytestmark = pytest.mark.gpu
KINDS = ("cancel", "nonfinite")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", route_cases.CASES, ids=[c["id"] for c in route_cases.CASES])
def test_route(c, kind):
    trace = t.launch_trace()
    with t.tuned(**c["keys"]):
        p = route_run.PREPARE[c["op"]](c, kind)
        with trace:
            p.call(torch.cuda.current_stream())
        torch.cuda.synchronize()
        launches = p.launches()
        p.close()
        p.check()
    print(f"{c['id']} {kind}:")
    route_run.check_trace(c, trace, launches)
