"""What polycap_source_get_transmission_efficiencies answers to a bad environment, string for string: tests/golden/call_refusals.json,
recorded from a build of this code kept outside the tree (scripts/record_call_refusals.py), against the tree's build.  Every refusal
happens before a device is used, so no GPU is needed.  The table pins the messages of every key of the POLYCAP_SPOT, _HIST, _JOINT,
_SELECT and _DRAW grammars, the 0|1 flags, POLYCAP_SELECT_RECORDS, POLYCAP_SPOT_SHARE and POLYCAP_HIP_DEVICES, what an empty value means, and with
two bad variables the order of validation: what a change to the host code of the call must keep, or reword on purpose (an entry marked
"changed" then carries the new message, and the recorded one as "recorded")."""
import json
import os

import pytest

from tests.conftest import EXAMPLE, ROOT

with open(os.path.join(ROOT, "tests", "golden", "call_refusals.json")) as f:
    TABLE = json.load(f)

VARIABLES = ["POLYCAP_STDERR", "POLYCAP_TALLY_STDERR", "POLYCAP_BEAM", "POLYCAP_SPOT", "POLYCAP_SPOT_SHARE", "POLYCAP_HIST", "POLYCAP_JOINT",
             "POLYCAP_SELECT", "POLYCAP_SELECT_RECORDS", "POLYCAP_DRAW", "POLYCAP_HIP_DEVICES", "POLYCAP_IMAGES"]
EXCEPTIONS = {"ValueError": ValueError}


def test_the_table_covers_what_it_is_meant_to():
    names = [e["name"] for e in TABLE]
    assert len(set(names)) == len(names) >= 100
    assert all(set(e["env"]) <= set(VARIABLES) and e["exception"] in EXCEPTIONS for e in TABLE)
    assert sum(1 for n in names if n.startswith("order-")) >= 6
    assert all("recorded" in e and "POLYCAP_SPOT_SHARE" in e["env"] for e in TABLE if e.get("changed"))


@pytest.mark.parametrize("entry", TABLE, ids=[e["name"] for e in TABLE])
def test_public_call_refuses_with_the_recorded_message(entry, monkeypatch):
    from polycap_amd import capi
    for name in VARIABLES:
        monkeypatch.delenv(name, raising=False)
    for name, value in entry["env"].items():
        monkeypatch.setenv(name, value)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(EXCEPTIONS[entry["exception"]]) as e:
        src.get_transmission_efficiencies(1, 1000, leak_calc=entry["leak_calc"])
    assert type(e.value) is EXCEPTIONS[entry["exception"]]
    assert str(e.value) == entry["message"]
