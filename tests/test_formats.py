"""The smaller output formats of the host-bound paths (include/gpsbb.h GPSBB_OUT_SC8 / GPSBB_OUT_SC1) on the CPU: the numpy
reference pack_iq on hand-worked vectors, gpsbb_out_bytes against numpy sizes and its refusals, and gpsbb-sim's refusal of a
format it does not write.  No GPU is touched."""
import os
import subprocess

import numpy as np
import pytest

# the issue's hand-worked components: both ends of int16, both sides of every shift boundary that matters, zero
V = [-32768, -17, -16, -1, 0, 1, 15, 16, 4095, 4096, 32767]


def sc8_by_hand(v, shift):
    """floor(v / 2^shift), saturated to int8"""
    q = v // (1 << shift)
    return max(-128, min(127, q))


@pytest.mark.parametrize("shift", [0, 4, 5, 15])
def test_pack_iq_sc8_floors_and_saturates(pkg, shift):
    iq = np.array(V + [0], np.int16).reshape(-1, 2)          # 12 components: I, Q, I, Q ...
    got = pkg.pack_iq(iq, pkg.OUT_SC8(shift))
    assert got.dtype == np.int8 and got.shape == iq.shape
    assert got.ravel().tolist() == [sc8_by_hand(v, shift) for v in V + [0]]


def test_pack_iq_sc8_worked_values(pkg):
    iq = np.array(V + [0], np.int16).reshape(-1, 2)
    assert pkg.pack_iq(iq, pkg.OUT_SC8(0)).ravel().tolist() == [-128, -17, -16, -1, 0, 1, 15, 16, 127, 127, 127, 0]
    assert pkg.pack_iq(iq, pkg.OUT_SC8(4)).ravel().tolist() == [-128, -2, -1, -1, 0, 0, 0, 1, 127, 127, 127, 0]
    assert pkg.pack_iq(iq, pkg.OUT_SC8(5)).ravel().tolist() == [-128, -1, -1, -1, 0, 0, 0, 0, 127, 127, 127, 0]
    assert pkg.pack_iq(iq, pkg.OUT_SC8(15)).ravel().tolist() == [-1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0]
    # a shift of 4 maps 4095 to 255 and -32768 to -2048: both saturate; 4096 >> 5 = 128 does as well
    assert int(pkg.pack_iq(np.array([[4095, -32768]], np.int16), pkg.OUT_SC8(4))[0, 0]) == 127


def test_pack_iq_sc1_msb_first_in_component_order(pkg):
    # 16 components = 8 samples = 2 bytes; component 8m is bit 7 of byte m, I before Q
    comps = V + [0, 2, -2, 3, 0]
    iq = np.array(comps, np.int16).reshape(-1, 2)
    got = pkg.pack_iq(iq, pkg.OUT_SC1)
    assert got.dtype == np.uint8 and got.shape == (2,)
    # byte 0: -32768 -17 -16 -1 0 1 15 16 -> 0 0 0 0 0 1 1 1; byte 1: 4095 4096 32767 0 2 -2 3 0 -> 1 1 1 0 1 0 1 0
    assert got.tolist() == [0b00000111, 0b11101010]
    # one positive I in the first sample is the top bit; one positive Q is the next
    one = np.zeros((4, 2), np.int16)
    one[0, 0] = 1
    assert pkg.pack_iq(one, pkg.OUT_SC1).tolist() == [0x80]
    one[0] = (0, 1)
    assert pkg.pack_iq(one, pkg.OUT_SC1).tolist() == [0x40]
    one[0] = (0, 0)
    one[3, 1] = 7
    assert pkg.pack_iq(one, pkg.OUT_SC1).tolist() == [0x01]


def test_pack_iq_blocks_pack_on_their_own(pkg):
    rng = np.random.default_rng(5)
    iq = rng.integers(-4000, 4000, size=(3, 20, 2)).astype(np.int16)
    flat = pkg.pack_iq(iq.reshape(1, 60, 2), pkg.OUT_SC1).reshape(3, 5)
    assert (pkg.pack_iq(iq, pkg.OUT_SC1) == flat).all()
    assert (pkg.pack_iq(iq, pkg.OUT_SC8(3)).reshape(-1) == pkg.pack_iq(iq.reshape(-1, 2), pkg.OUT_SC8(3)).reshape(-1)).all()
    assert (pkg.pack_iq(iq, pkg.OUT_SC16) == iq).all()
    with pytest.raises(ValueError):
        pkg.pack_iq(iq[:, :18], pkg.OUT_SC1)                 # nsamp % 4 != 0


@pytest.mark.parametrize("nsamp", [1, 3, 4, 7, 8, 300000, 2500000, 262146])
def test_out_bytes_matches_numpy(pkg, nsamp):
    L = pkg.lib()
    iq = np.zeros((nsamp, 2), np.int16)
    assert L.gpsbb_out_bytes(pkg.OUT_SC16, nsamp) == iq.nbytes == pkg.out_bytes(pkg.OUT_SC16, nsamp)
    for shift in (0, 5, 15):
        assert L.gpsbb_out_bytes(pkg.OUT_SC8(shift), nsamp) == pkg.pack_iq(iq, pkg.OUT_SC8(shift)).nbytes
    if nsamp % 4 == 0:
        assert L.gpsbb_out_bytes(pkg.OUT_SC1, nsamp) == pkg.pack_iq(iq, pkg.OUT_SC1).nbytes == nsamp // 4
    else:
        assert L.gpsbb_out_bytes(pkg.OUT_SC1, nsamp) == -1
    # the flags below the format (GPSBB_CHAIN_CARRIER, GPSBB_FIXED_CARRIER, GPSBB_STREAM_DEVICE_ONLY ...) do not change the size
    assert L.gpsbb_out_bytes(pkg.OUT_SC8(4) | pkg.CHAIN_CARRIER | pkg.FIXED_CARRIER, nsamp) == 2 * nsamp


def test_out_bytes_refusals(pkg):
    L = pkg.lib()
    assert pkg.OUT_SC8(0) == 0x100 and pkg.OUT_SC8(15) == 0xF100 and pkg.OUT_SC1 == 0x200
    assert L.gpsbb_out_bytes(pkg.OUT_SC8(16), 100) == -1          # a shift above 15
    assert L.gpsbb_out_bytes(3 << 8, 100) == -1                   # unknown formats
    assert L.gpsbb_out_bytes(15 << 8, 100) == -1
    assert L.gpsbb_out_bytes(pkg.OUT_SC1 | (1 << 12), 100) == -1  # a shift is SC8's alone
    assert L.gpsbb_out_bytes(1 << 12, 100) == -1
    assert L.gpsbb_out_bytes(pkg.OUT_SC1, 102) == -1              # SC1: nsamp % 4 == 0
    assert L.gpsbb_out_bytes(pkg.OUT_SC16, 0) == -1
    assert L.gpsbb_out_bytes(pkg.OUT_SC8(4), -4) == -1
    with pytest.raises(pkg.GpsbbError):
        pkg.out_bytes(pkg.OUT_SC8(16), 100)


@pytest.mark.parametrize("bits", ["4", "2", "0", "32", "x"])
def test_gpsbb_sim_refuses_other_sample_formats(pkg, tmp_path, bits):
    """-b takes 1, 8 or 16; anything else is a usage error before a GPU or a file is touched"""
    pkg.build_frontend()
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "gpsbb-sim")
    out = tmp_path / "never.bin"
    r = subprocess.run([exe, "-e", "/nonexistent.14n", "-b", bits, "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage" in r.stderr
    assert not out.exists()
    r = subprocess.run([exe, "-e", "/nonexistent.14n", "-b", "8", "-q", "16", "-o", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "usage" in r.stderr
