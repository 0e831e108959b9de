"""What a received record brings to the return cube, on the host (no GPU): rts_amd/csrc/rts_cube_source.h alone (tests/cube_source/
cube_source_main.cpp, g++ -O2 -ffp-contract=off, and again under AddressSanitizer + UndefinedBehaviorSanitizer) -- which record counts
for a receiver, with which delay and phase -- against numpy bit for bit and against tests/cube_ref.py; and the plan of the Doppler
map's launch and the transforms' log2 (rts_amd/csrc/rts_stft.h) against the three lines the launcher used to spell out.

Bit for bit: the delay is ONE division, the phase two multiplications by doubles, one exact fmod and a sign -- IEEE basic operations
in the reference's operand order (aggregation.cu:59-60), which numpy's float64 performs one at a time.  The amplitude goes through
libm's sin and cos on one side and numpy's on the other: each within an ulp of the true value, so the components agree to
4 x 2^-52 sqrt(P)."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cube_ref  # noqa: E402

N_RX = 3
CSPEED, CARRIER = 299792458.0, 9.6e9
BIG_BASE = 2 ** 31 - 20                       # a row base at the end of int32: base + i passes 2^31 at record 20 and is formed in 64 bits


def build(tmp, name, flags):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + ["-I", os.path.join(ROOT, "rts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cube_source", "cube_source_main.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """the driver as the library's host code is built (-O2), and under the sanitizers where g++ has them"""
    tmp = tmp_path_factory.mktemp("cube_source")
    gxx = shutil.which("g++")
    exes = [build(tmp, "plain", ["-O2"])]
    rt = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(rt) and os.path.exists(rt):
        exes.append(build(tmp, "sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def ask(lines):
        outs = []
        for exe in exes:
            r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, env=env, timeout=120)
            assert r.returncode == 0, r.stderr[-3000:]
            outs.append(r.stdout.splitlines())
            assert len(outs[-1]) == len(lines)
        assert all(o == outs[0] for o in outs), "the plain and the sanitized build differ"
        return outs[0]
    return ask


def record_set(base):
    """about 40 hand-made records: (received, rayLength, power, pathMatch, group delay, group phase).  Receivers -1, 0, N_RX - 1 and
    N_RX; pathMatch equal and unequal to base + i; a zero, an infinite and a NaN ray length; group phases on both sides of zero"""
    recs = []
    for i in range(40):
        rx = (-1, 0, 1, N_RX - 1, N_RX)[i % 5]
        length = 150.0 + 37.03125 * i + (i % 7) * 1.0e-3
        if i == 6:
            length = 0.0
        if i == 12:
            length = math.inf
        if i == 18:
            length = math.nan
        pm = base + i if i % 3 != 1 else base + (i - 1)              # every third ray belongs to its predecessor's group
        if i == 25:
            pm = -1                                                  # the reference's "no group"
        pm = ((pm + 2 ** 31) % 2 ** 32) - 2 ** 31                    # as the int32 the array holds: past 2^31 the low 32 bits of base + i
        recs.append((rx, length, 1.0e-9 * (1 + i % 11), pm, 1.0e-6 + 3.3e-9 * i, (i - 20) * 0.37))
    return recs


def ask_read(drivers, recs, paths, base, rx):
    line = "read %d %d %d %d %r %r %d " % (paths, base, N_RX, rx, CSPEED, CARRIER, len(recs))
    line += " ".join("%d %r %r %d %r %r" % r for r in recs)
    f = drivers([line])[0].split()
    assert len(f) == 7 * len(recs)
    return [(int(f[7 * i]), int(f[7 * i + 1]), int(f[7 * i + 2]), int(f[7 * i + 3]), int(f[7 * i + 4]), float(f[7 * i + 5]), float(f[7 * i + 6])) for i in range(len(recs))]


def bits(x):
    return int(np.float64(x).view(np.uint64))


@pytest.mark.parametrize("base", [0, BIG_BASE])
@pytest.mark.parametrize("paths", [0, 1])
def test_read_against_numpy(drivers, paths, base):
    recs = record_set(base)
    assert {r[0] for r in recs} == {-1, 0, 1, N_RX - 1, N_RX}
    for rx in (-1, 0, N_RX - 1, N_RX):
        got = ask_read(drivers, recs, paths, base, rx)
        counted = 0
        for i, (r, g) in enumerate(zip(recs, got)):
            received, length, power, pm, gdelay, gphase = r
            # pathMatch is an int32 and base + i is not: equal only as 64-bit integers (past 2^31 only their low 32 bits agree)
            rep = (not paths) or pm == base + i
            want_asked = received == rx and rep
            want_any = 0 <= received < N_RX and rep
            assert (g[0], g[1]) == (int(want_asked), int(want_any)), (i, r, g)
            assert g[2] == received
            if not (want_asked or want_any):
                continue
            counted += 1
            with np.errstate(all="ignore"):
                if paths:
                    delay, phase = np.float64(gdelay), np.float64(gphase)
                else:
                    delay = np.float64(length) / np.float64(CSPEED)
                    phase = -np.fmod(delay * 2 * np.pi * np.float64(CARRIER), 2 * np.pi)
            if math.isnan(delay):
                assert math.isnan(np.uint64(g[3]).view(np.float64)) and math.isnan(np.uint64(g[4]).view(np.float64)), (i, g)
                continue
            assert g[3] == bits(delay), (i, r, g)
            if math.isnan(phase):                                        # an infinite delay: fmod(inf, .) is NaN
                assert math.isinf(delay) and math.isnan(np.uint64(g[4]).view(np.float64))
                continue
            assert g[4] == bits(phase), (i, r, g)
            amp = math.sqrt(power)
            assert abs(g[5] - amp * math.cos(float(phase))) <= 4 * 2.0 ** -52 * amp and abs(g[6] - amp * math.sin(float(phase))) <= 4 * 2.0 ** -52 * amp
        assert counted >= (2 if paths else 8) or rx == N_RX
    if paths:
        assert recs[25][3] != base + 25 and recs[0][3] == base and (base == 0 or recs[21][3] == base + 21 - 2 ** 32)


def test_read_against_cube_ref(drivers):
    """the restatement the GPU tests use: the same records count, with the same delay, and the amplitude agrees to the bound of
    the two phases: x = 2 pi fc tau is formed with two roundings in float64 and none to speak of in longdouble, pi and the modulus
    2 pi are the float64 ones on one side and the longdouble ones on the other (0.35 x 2^-53 x each): below 4 x 2^-53 x in all"""
    recs = record_set(0)
    records = np.zeros(len(recs), dtype=[("received", "i4"), ("rayLength", "f8"), ("power", "f8"), ("doppler", "f8")])
    for i, r in enumerate(recs):
        records[i] = (r[0], r[1], r[2], 0.0)
    with np.errstate(all="ignore"):
        rays = cube_ref.contribs_rays(records, CSPEED, CARRIER)
    got = ask_read(drivers, recs, 0, 0, 0)
    for i, (c, g) in enumerate(zip(rays, got)):
        rx, a, tau, _f = c
        assert g[1] == int(0 <= rx < N_RX) and g[2] == rx
        if not g[1] or not math.isfinite(tau):
            continue
        assert g[3] == bits(tau)
        tol = (4 * 2.0 ** -53 * 2 * math.pi * CARRIER * tau + 8 * 2.0 ** -52) * math.sqrt(recs[i][2])
        assert abs(complex(g[5], g[6]) - complex(a)) <= tol, (i, g, a)
    paths = cube_ref.contribs_paths([r[0] for r in recs], [r[2] for r in recs], [0.0] * len(recs), [r[4] for r in recs], [r[5] for r in recs], [r[3] for r in recs])
    got = ask_read(drivers, recs, 1, 0, 0)
    kept = [i for i in range(len(recs)) if recs[i][3] == i]
    assert len(paths) == len(kept) and 20 < len(kept) < 40
    for c, i in zip(paths, kept):
        rx, a, tau, _f = c
        g = got[i]
        assert g[1] == int(0 <= rx < N_RX)
        if g[1]:
            assert g[3] == bits(tau) and g[4] == bits(recs[i][5])
            assert abs(complex(g[5], g[6]) - complex(a)) <= 8 * 2.0 ** -52 * math.sqrt(recs[i][2])
    dropped = [i for i in range(len(recs)) if i not in kept]
    assert all(got[i][0] == 0 and got[i][1] == 0 for i in dropped)


def test_empty_set(drivers):
    assert drivers(["read 0 0 3 0 %r %r 0" % (CSPEED, CARRIER), "read 1 7 3 0 %r %r 0" % (CSPEED, CARRIER)]) == ["", ""]


def test_doppler_plan_is_the_launchers_three_lines(drivers):
    """rts_cube_doppler_device used to read: logN = 0; while ((1 << logN) < n_fft) logN++;  BT = 8; while (BT > 1 && n_fft * BT * 16 >
    65536) BT >>= 1;  lds = n_fft * BT * 16 + n_fft * 8"""
    sizes = [2 << e for e in range(12)]
    assert sizes[0] == 2 and sizes[-1] == 4096
    for n_fft, line in zip(sizes, drivers(["dopplerplan %d" % n for n in sizes])):
        logN = 0
        while (1 << logN) < n_fft:
            logN += 1
        BT = 8
        while BT > 1 and n_fft * BT * 16 > 65536:
            BT >>= 1
        assert [int(x) for x in line.split()] == [logN, BT, n_fft * BT * 16 + n_fft * 8], n_fft
    assert drivers(["dopplerplan 1024"]) == ["10 4 %d" % (64 * 1024 + 8 * 1024)] and drivers(["dopplerplan 4096"]) == ["12 1 %d" % (96 * 1024)]


def test_log2_is_the_ceiling(drivers):
    """the least logN with 2^logN >= n: (n - 1).bit_length(), for 1 .. 2^31 (the powers of two, their neighbours, and a spread)"""
    rng = np.random.default_rng(5)
    ns = sorted({1, 2, 3} | {(1 << k) + d for k in range(2, 32) for d in (-1, 0, 1) if (1 << k) + d <= 2 ** 31} | {int(x) for x in rng.integers(1, 2 ** 31, 200)})
    assert ns[0] == 1 and ns[-1] == 2 ** 31
    got = [int(x) for x in drivers(["log2 " + " ".join(str(n) for n in ns)])[0].split()]
    assert got == [(n - 1).bit_length() for n in ns]
