"""CPU check of what the ten frame entries refuse before they touch the device: tests/golden/frame_screening.json (written by
tests/golden/make_frame_screening.py from the library before the frame entries were folded into one argument record, one input
prelude and one history screen) replayed call by call under error mode 1.  A case (the generator's cases()) is an entry, the thread settings to
apply and an argument list of dummy addresses; the file holds, per case, the text of stm_last_error() after its first line (the fail site's file:line): the message,
the entry's name in it and the rule that wins where two are broken must all stay as recorded.  No compute call -- every case
is refused by the entry's own screen, which the table's generator and the test below both insist on."""
import importlib.util
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_frame_screening", os.path.join(GOLDEN, "make_frame_screening.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

TABLE = gen.load_table()  # {(entry, label): message}


@pytest.fixture
def lib(stm):
    from stm_amd import _lib
    lib = stm.lib()
    lib.stm_set_error_mode(1)
    try:
        yield lib
    finally:
        gen.apply_settings(lib, _lib.PROTOS, gen.RESET)  # (every case restores them itself as well)
        lib.stm_set_error_mode(0)


def test_the_table_is_the_generators_cases():
    """the committed table holds a message for exactly the cases the generator builds now, for all ten entries"""
    keys = [(c["entry"], c["label"]) for c in gen.cases()]
    assert len(set(keys)) == len(keys) and set(keys) == set(TABLE)
    assert {e for e, _ in TABLE} == set(gen.ENTRIES) and len(gen.ENTRIES) == 10


@pytest.mark.parametrize("entry", sorted(gen.ENTRIES))
def test_refusals_are_as_recorded(lib, entry):
    from stm_amd import _lib
    from stm_amd import device_api as dev
    rows = [c for c in gen.cases() if c["entry"] == entry]
    assert len(rows) > 40
    for c in rows:
        want = TABLE[(entry, c["label"])]
        assert want.startswith(entry[4:] + ": "), c["label"]  # the entry's own screen: nothing was launched or written
        assert gen.refusal(lib, _lib.PROTOS, c) == want, c["label"]
        # the case's settings are gone again
        assert dev.get_packing() == (0, 0, 0, 0) and dev.get_align()[0] == 0 and dev.get_balance()[0] == 0 and dev.get_cut()[0] == 0
        assert dev.get_layout()[0] == 0 and dev.get_output()[0] == 0 and dev.get_overlay()[0] == 0
