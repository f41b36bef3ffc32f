"""PathTracer makes the same calls on its context as it did before its frame chain was unified: the script of
tests/golden/gen_frame_trace.py, replayed on a recording context, equals the trace recorded from that commit (frame_trace.json)."""
import importlib.util
import json
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"


def test_pathtracer_calls_match_the_recorded_trace():
    spec = importlib.util.spec_from_file_location("gen_frame_trace", GOLDEN / "gen_frame_trace.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.loads((GOLDEN / "frame_trace.json").read_text())
    got = gen.record()
    assert len(want) > 500 and {"launch", "create", "upload", "handles"} <= {e[0] for e in want}
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"event {i}: {g} != {w} (after {[e for e in want[:i] if e[0] == 'step'][-1:]})"
    assert len(got) == len(want)
