"""The byte layout gpsbb_fill_block_ref is tested with (conftest.REF_CHANNEL_DTYPE) against the REAL channel_t: offsetof()
of every field the entry point touches, plus sizeof(channel_t), as a C program including the reference's plutogpssim.h
printed them (tests/golden/make_ref_layout.py -> tests/golden/ref_channel_t_layout.json)."""
import json
import os

import pytest

from conftest import GOLDEN, REF_CHANNEL_DTYPE, REF_CHANNEL_FIXED_DTYPE

LAYOUT = os.path.join(GOLDEN, "ref_channel_t_layout.json")
FIELDS = ["prn", "ca", "f_carr", "f_code", "carr_phase", "code_phase", "g0", "sbf", "dwrd", "iword", "ibit", "icode",
          "dataBit", "codeCA", "azel", "rho0"]


@pytest.mark.parametrize("fixed", [False, True])
def test_channel_t_offsets(fixed):
    """fixed: the header with line 12 (`#define FLOAT_CARR_PHASE`) taken out — the reference's other channel_t (h:160-161),
    the layout gpsbb_fill_block_ref_fixed reads."""
    fields, dtype = list(FIELDS), REF_CHANNEL_DTYPE
    if fixed:
        fields.insert(fields.index("carr_phase") + 1, "carr_phasestep")
        dtype = REF_CHANNEL_FIXED_DTYPE
    got = json.load(open(LAYOUT))["fixed_carr_phase" if fixed else "float_carr_phase"]
    assert sorted(got["offsets"]) == sorted(fields)
    name = {"g0": "g0_week"}
    for f in fields:
        assert got["offsets"][f] == dtype.fields[name.get(f, f)][1], f
    assert got["sizeof"] == dtype.itemsize
    assert got["sizeof_dwrd_elem"] == 8
    assert got["sizeof_carr_phase"] == (4 if fixed else 8)
