"""CPU check of what the stage entries and the thread setters refuse before they touch the device: tests/golden/entry_screening.json
(written by tests/golden/make_entry_screening.py from the library of the commit its first row names, before the refusal sites were
folded through one helper) replayed call by call under error mode 1.  A case (the generator's cases()) is an entry and an argument
list of dummy addresses; the file holds, per case, the text of stm_last_error() after its first line (the fail site's file:line):
the message, the entry's name in it and the rule that wins where two are broken must all stay as recorded.  No compute call --
every case is refused by the entry's own screen, which the table's generator and the test below both insist on."""
import importlib.util
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_entry_screening", os.path.join(GOLDEN, "make_entry_screening.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

TABLE, COMMIT = gen.load_table()  # {(entry, label): text}
CASES = gen.cases()


@pytest.fixture
def lib(stm):
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        yield lib
    finally:
        lib.stm_set_error_mode(0)


def test_the_table_is_the_generators_cases():
    """the committed table holds a message for exactly the cases the generator builds now, and names the commit it was recorded from"""
    keys = [(c["entry"], c["label"]) for c in CASES]
    assert len(set(keys)) == len(keys) and set(keys) == set(TABLE)
    assert len(COMMIT) == 40 and int(COMMIT, 16) >= 0


def test_every_exported_entry_is_screened_somewhere():
    """_lib.PROTOS is this table's entries, the frame table's, the stream entries (stream_screening.json) and the generator's explicit
    list of entries that refuse nothing: a stage or a setter added later has to join one of them"""
    from stm_amd import _lib
    stream = {n for n in _lib.PROTOS if n.startswith(gen.STREAM_PREFIX)}
    groups = [set(gen.ENTRIES), gen.FRAME_ENTRIES, stream, gen.NO_SCREEN]
    assert sum(len(g) for g in groups) == len(set().union(*groups))  # disjoint
    assert set().union(*groups) == set(_lib.PROTOS)
    # every stage and every thread setter of the header is in the table itself
    assert {n for n in _lib.PROTOS if n.startswith("stm_set_") and n not in gen.NO_SCREEN} <= set(gen.ENTRIES)
    assert set(gen.STREAM_SETTERS) == {n for n in stream if n.startswith("stm_stream_set_")} | {"stm_stream_overlay"}


@pytest.mark.parametrize("entry", sorted(gen.ENTRIES))
def test_refusals_are_as_recorded(lib, entry):
    from stm_amd import _lib
    from stm_amd import device_api as dev
    rows = [c for c in CASES if c["entry"] == entry]
    assert rows

    def replay():  # on a thread of its own: the settings start from their defaults whatever ran before
        for c in rows:
            want = c["says"] + ": " + TABLE[(entry, c["label"])]
            assert c["says"] == entry[4:] or c["says"] == "mux_multiview", c["label"]  # the entry's own screen: nothing was launched or written
            assert gen.run(lib, _lib.PROTOS, c) == want, c["label"]
            # a refused setter leaves its setting alone, and the case's reset leaves the defaults
            assert dev.get_packing() == (0, 0, 0, 0) and dev.get_align()[0] == 0 and dev.get_balance()[0] == 0 and dev.get_cut()[0] == 0
            assert dev.get_layout()[0] == 0 and dev.get_output()[0] == 0 and dev.get_overlay()[0] == 0 and dev.get_active()[0] == 0
            assert dev.get_antialias()[0] == 0 and dev.get_overlay_auto()[0] == 0
    gen.in_fresh_thread(replay)
