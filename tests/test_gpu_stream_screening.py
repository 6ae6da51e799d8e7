"""What the stream setters refuse: tests/golden/stream_screening.json (written by tests/golden/make_entry_screening.py --stream from the
library of the commit its first row names) replayed call by call under error mode 1 -- the companion of test_entry_screening.py for
the entries that need a stream, so a device.  A case (the generator's stream_cases()) is a setter, its arguments, the setter calls
that prepare the stream and whether a frame has gone through it; the streams are of a 40 x 64 frame.  Every case is refused by
host code: the call returns -1 with the recorded text, the rule that wins where two are broken included, and launches nothing."""
import importlib.util
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_entry_screening", os.path.join(GOLDEN, "make_entry_screening.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

TABLE, COMMIT = gen.load_table(gen.OUT_STREAM)  # {(entry, label): text}
CASES = gen.stream_cases()


def test_the_table_is_the_generators_cases():
    """the committed table holds a message for exactly the cases the generator builds now; every setter with the rule has its
    "only before the first submit" case, alone and behind a broken argument"""
    keys = [(c["entry"], c["label"]) for c in CASES]
    assert len(set(keys)) == len(keys) and set(keys) == set(TABLE)
    assert len(COMMIT) == 40 and int(COMMIT, 16) >= 0
    for name in gen.STREAM_SETTERS:
        if name != "stm_stream_overlay":
            assert TABLE[(name, "after-submit")].startswith("only before the first submit"), name
            assert not TABLE[(name, "broken+after-submit")].startswith("only before the first submit"), name


def test_refusals_are_as_recorded(gpu_ready, stm):
    from stm_amd import _lib
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    streams = gen.Streams(lib, _lib.PROTOS)
    try:
        for c in CASES:
            rc, msg = streams.run(c)
            assert rc == -1 and msg == c["says"] + ": " + TABLE[(c["entry"], c["label"])], (c["entry"], c["label"])
    finally:
        streams.close()
        lib.stm_set_error_mode(0)
