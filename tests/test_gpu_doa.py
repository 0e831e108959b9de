"""Direction finding on the device (rts_cube_eig, rts_cube_doa_scan): the kernels against the host evaluators rts_eig_eval /
rts_doa_scan_eval BIT FOR BIT (the trees hold + - * /, sqrt and comparisons only) over the smallest shapes at which they can go wrong.
k_eig: orders 1 .. 5; the rotation's rows are dealt to RTS_EIG_LANES = 8 lanes per pair (rts_amd/csrc/rts_doa.h), so 7, 8, 9 rows (a
lane without a row, a row each, a second row) and 15, 16, 17; 8 pairs fill a wave, so 16 and 32 (a wave, two waves of pairs) with
their neighbours 31, 33; the limit 63, 64 (32 pairs: the whole workgroup) -- a pair's SUMS are not split across lanes, so the tree
has no partition to test --; full-rank, rank-deficient, identity and diagonal inputs, the three covariance sources, the status rules.  k_doa_scan: directions around the wave and the workgroup, vectors around the
vector tile, elements around the element tile, a row range inside a table whose other rows are NaN, NaN around the steering table and
sentinels around a caller-owned output, the inverse flag with q = 0, run-to-run equality, the beamformer's power.  The two-source
scenario of tests/doa_ref.py through Tracer.cube_doa against its host chain, and the error / lifetime rules on a live handle."""
import ctypes as C
import math

import numpy as np
import pytest

import beam_ref as B
import doa_ref as D

pytestmark = pytest.mark.gpu
WG, VT, RXT = D.SCAN_THREADS, D.VEC_TILE, D.RX_TILE


def dev(a, dtype=np.complex128):
    """(torch's stream is not the handles': the buffer is finished before a handle reads it, and a handle's work before torch reads it)"""
    import torch
    buf = torch.from_numpy(np.array(a, dtype, order="C")).to("cuda")
    torch.cuda.synchronize()
    return buf


def host(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def handle(rts, n_rx=1):
    tr = rts.Tracer(8, 1)
    tr.cube_attach(n_rx, 1, 1, 0.0, 1.0)
    return tr


# ----------------------------------------------------------------------------- 1. the solve against the evaluator
@pytest.mark.parametrize("kind", ["full", "deficient", "identity", "diagonal"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64])
def test_eig_against_the_evaluator(rts, n, kind):
    A = D.matrix(kind, n)
    poisoned = A.copy(); poisoned[np.triu_indices(n, 1)] = np.nan                  # the upper triangle and the diagonal's imaginary parts: never read
    poisoned.view(np.float64).reshape(n, n, 2)[np.arange(n), np.arange(n), 1] = np.nan
    dc = dev(poisoned)
    tr = handle(rts)
    values, vectors = tr.cube_eig(n=n, device_cov=dc.data_ptr())                   # (the getter succeeds: status 0)
    want_values, want_vectors = rts.eig_eval(A)
    assert values.shape == (n,) and vectors.shape == (n, n) and np.all(np.isfinite(values)) and np.all(np.isfinite(bits(vectors)))
    assert np.array_equal(bits(values), bits(want_values)) and np.array_equal(bits(vectors), bits(want_vectors)), (n, kind)
    tr.close()


def test_eig_covariance_sources_and_outputs(rts):
    rng = np.random.default_rng(77)
    inp = B.random_complex(rng, (3, 9, 21))
    d = dev(inp)
    tr = rts.Tracer(8, 1); tr.cube_attach(3, 9, 21, 0.0, 1.0, device_ptr=d.data_ptr())
    train = dict(first=1, count=7, first_bin=2)
    tr.cube_covariance(fetch=False, **train)                                        # the receivers' covariance, library-owned
    got = tr.cube_eig()
    want = rts.eig_eval(rts.covariance_eval(inp, **train))
    assert got[0].shape == (3,) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want))
    tr.cube_st_covariance(2, fetch=False, **train)                                  # the stacked one of order 2 x 3, unchanged
    got = tr.cube_eig()
    cov6 = rts.st_covariance_eval(inp, 2, **train)
    want = rts.eig_eval(cov6)
    assert got[0].shape == (6,) and got[1].shape == (6, 6) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want))
    # device_cov, into caller-owned outputs between sentinels; the library-owned eigenpairs stay what they were
    import torch
    dc = dev(cov6)
    vals = torch.full((6 + 2,), -7.0, dtype=torch.float64, device="cuda"); vecs = torch.full((2 * (36 + 2),), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert tr.cube_eig(n=6, device_cov=dc.data_ptr(), device_values=vals.data_ptr() + 8, device_vectors=vecs.data_ptr() + 16) is None
    again = tr.eigenpairs()                                                         # (the getter waits for the handle's stream)
    hv, hx = host(vals), host(vecs)
    assert hv[0] == -7.0 and hv[-1] == -7.0 and np.all(hx[:2] == -7.0) and np.all(hx[-2:] == -7.0)
    assert np.array_equal(hv[1:-1], want[0]) and np.array_equal(hx[2:-2], bits(want[1]).ravel())
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(again, want))
    tr.close()


def test_eig_status_2(rts):
    """a NaN in the lower triangle: every output NaN, the getter's error names the status, and the handle goes on working"""
    import torch
    n = 5
    A = D.matrix("full", n)
    bad = A.copy(); bad[3, 1] = complex(1.0, np.nan)
    tr = handle(rts)
    db = dev(bad)
    with pytest.raises(rts.L.RtsError) as e:
        tr.cube_eig(n=n, device_cov=db.data_ptr())
    assert e.value.code == rts.L.RTS_ERR_INVALID and "status 2" in str(e.value)
    vals = torch.zeros(n, dtype=torch.float64, device="cuda"); vecs = torch.zeros(2 * n * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    tr.cube_eig(n=n, device_cov=db.data_ptr(), device_values=vals.data_ptr(), device_vectors=vecs.data_ptr())
    with pytest.raises(rts.L.RtsError):
        tr.eigenpairs()                                                             # (still the library-owned solve's status; it waits for the stream)
    assert np.all(np.isnan(host(vals))) and np.all(np.isnan(host(vecs)))
    inf = A.copy(); inf[2, 2] = np.inf
    di = dev(inf)
    with pytest.raises(rts.L.RtsError):
        tr.cube_eig(n=n, device_cov=di.data_ptr())
    da = dev(A)
    got = tr.cube_eig(n=n, device_cov=da.data_ptr())                                # the handle is as usable as before
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, rts.eig_eval(A)))
    tr.close()


def test_eig_run_to_run(rts):
    A = D.matrix("full", 33)
    da = dev(A)
    tr = handle(rts)
    first = tr.cube_eig(n=33, device_cov=da.data_ptr())
    for _ in range(3):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(tr.cube_eig(n=33, device_cov=da.data_ptr()), first))
    tr.close()


# ----------------------------------------------------------------------------- 2. the scan against the evaluator
def scan_inputs(n, n_dirs, seed):
    """(vector table [n][n], host steering table [n_dirs][n], the device buffer [NaN | element-major table | NaN], its table's pointer)"""
    rng = np.random.default_rng(seed)
    vectors = B.random_complex(rng, (n, n)); table = B.random_complex(rng, (n_dirs, n))
    pad = np.full(3, np.nan + 1j * np.nan)
    buf = dev(np.concatenate([pad, np.ascontiguousarray(table.T).ravel(), pad]))
    return vectors, table, buf, buf.data_ptr() + 16 * len(pad)


# (n, m, first_vector, n_dirs, inverse): the wave (63, 64, 65) and the workgroup (WG - 1, WG, WG + 1) of directions; 1, the vector
# tile's edges and n vectors; 1, 2, the element tile's edges, 21 and 64 elements
SCAN_CASES = [(1, 1, 0, 1, False), (2, 1, 1, 63, True), (2, 2, 0, 64, False), (RXT - 1, 3, 2, 65, True), (RXT, RXT, 0, 65, False), (RXT + 1, 2, 7, 64, True),
              (21, 1, 20, 65, True), (21, VT - 1, 3, WG - 1, False), (21, VT, 5, WG, True), (21, VT + 1, 4, WG + 1, False), (21, 21, 0, 64, True),
              (64, 1, 0, 65, False), (64, VT - 1, 49, 63, True), (64, VT, 48, WG + 1, False), (64, VT + 1, 47, WG, True), (64, 62, 2, 300, True), (64, 64, 0, 129, False)]


@pytest.mark.parametrize("n,m,first,n_dirs,inverse", SCAN_CASES)
def test_scan_against_the_evaluator(rts, n, m, first, n_dirs, inverse):
    import torch
    vectors, table, buf, table_ptr = scan_inputs(n, n_dirs, 7919 * n + 31 * m + n_dirs)
    g = np.random.default_rng(m).random(m) + 0.25
    want = rts.doa_scan_eval(vectors[first:first + m], g, table, inverse)
    poisoned = np.full((n, n), np.nan + 1j * np.nan); poisoned[first:first + m] = vectors[first:first + m]          # the rows outside the range are never read
    dv = dev(poisoned)
    tr = handle(rts)
    kw = dict(first_vector=first, inverse=inverse, n_dirs=n_dirs, device_vectors=dv.data_ptr(), n=n)
    got = tr.cube_doa_scan(table_ptr, g, **kw)
    assert got.shape == (n_dirs,) and np.all(np.isfinite(got))
    assert np.array_equal(bits(got), bits(want)), (n, m, first, n_dirs, inverse)
    out = torch.full((n_dirs + 2,), -7.0, dtype=torch.float64, device="cuda")      # a caller-owned output between sentinels, 8-byte aligned
    torch.cuda.synchronize()
    assert tr.cube_doa_scan(table_ptr, g, device_ptr=out.data_ptr() + 8, **kw) is None
    assert np.array_equal(bits(tr.doa_spectrum()), bits(want))                     # (waits for the stream; the library-owned output is still the first call's)
    h = host(out)
    assert h[0] == -7.0 and h[-1] == -7.0 and np.array_equal(bits(h[1:-1]), bits(want))
    for _ in range(2):
        assert np.array_equal(bits(tr.cube_doa_scan(table_ptr, g, **kw)), bits(want))         # run to run
    tr.close()


def test_scan_inverse_of_zero_is_inf(rts):
    vectors = np.array([[1.0, -1.0], [1.0, 1.0]], np.complex128)
    table = np.array([[1.0, 1.0], [1.0, 0.0], [2.0, 2.0]], np.complex128)          # directions 0 and 2 are orthogonal to vector 0
    tr = handle(rts)
    dv = dev(vectors)
    got = tr.cube_doa_scan(table, [1.0], inverse=True, device_vectors=dv.data_ptr(), n=2)     # a host table: uploaded by the wrapper
    assert got[0] == math.inf and got[2] == math.inf and got[1] == 1.0
    assert np.array_equal(bits(got), bits(rts.doa_scan_eval(vectors[:1], [1.0], table, True)))
    tr.close()


@pytest.mark.parametrize("n", [3, 8, 21, 64])
def test_scan_of_one_vector_is_the_beamformer_on_the_device(rts, n):
    rng = np.random.default_rng(n)
    n_dirs = 2 * WG + 37
    table = B.random_complex(rng, (n_dirs, n)); w = B.random_complex(rng, (1, n))
    cube = np.ascontiguousarray(table.T)[:, None, :]                               # the table as a cube of one row whose bins are the directions
    d = dev(cube)
    tr = rts.Tracer(8, 1); tr.cube_attach(n, 1, n_dirs, 0.0, 1.0, device_ptr=d.data_ptr())
    beams = tr.cube_beamform(w, power=True)[0, 0]
    tab = np.zeros((n, n), np.complex128); tab[0] = w[0]
    dv = dev(tab)
    got = tr.cube_doa_scan(d.data_ptr(), [1.0], n_dirs=n_dirs, device_vectors=dv.data_ptr(), n=n)
    assert np.array_equal(bits(got), bits(beams))
    tr.close()


def test_scan_of_library_owned_eigenvectors(rts):
    """rts_cube_eig's library-owned table, a row range of it, and n = 0 or the table's order"""
    rng = np.random.default_rng(12)
    n = 6
    A = D.matrix("full", n); table = B.random_complex(rng, (70, n))
    da = dev(A)
    tr = handle(rts)
    values, vectors = tr.cube_eig(n=n, device_cov=da.data_ptr())
    for first, m in [(0, n), (2, 4), (5, 1)]:
        g = np.arange(1.0, m + 1.0)
        want = rts.doa_scan_eval(vectors[first:first + m], g, table, True)
        assert np.array_equal(bits(tr.cube_doa_scan(table, g, first_vector=first, inverse=True)), bits(want))
        assert np.array_equal(bits(tr.cube_doa_scan(table, g, first_vector=first, inverse=True, n=n)), bits(want))
    tr.close()


# ----------------------------------------------------------------------------- 3. the scenario through Tracer.cube_doa
@pytest.fixture(scope="module")
def scene(rts):
    cube = D.scene_cube(rts)
    pos, directions = D.scene_geometry()
    return cube, rts.steering(pos, directions, D.SCENE["wavelength"])


@pytest.mark.parametrize("method,n_sources", [("bartlett", None), ("capon", None), ("music", 2), ("music", None)])
def test_scenario_on_the_device(rts, scene, method, n_sources):
    cube, table = scene
    d = dev(cube)
    tr = rts.Tracer(8, 1); tr.cube_attach(cube.shape[0], 1, cube.shape[2], 0.0, 1.0, device_ptr=d.data_ptr())
    got = tr.cube_doa(table, method=method, n_sources=n_sources)
    want, _ = D.scene_host(rts, method, n_sources)
    assert np.array_equal(bits(got), bits(want)), method
    grid = np.degrees(D.SCENE["grid"]); pk = D.peaks(got)
    if method == "bartlett":
        assert len(pk) == 1
    else:
        assert len(pk) == 2 and (method != "music" or (abs(grid[pk[0]] + 3.0) <= 0.25 + 1e-9 and abs(grid[pk[1]] - 3.0) <= 0.25 + 1e-9))
    tr.close()


# ----------------------------------------------------------------------------- 4. errors and lifetime on a live handle
def test_refusals_and_lifetime(rts):
    import torch
    L = rts.L; lib = L.lib()
    n = 4
    A = D.matrix("full", n); table = B.random_complex(np.random.default_rng(1), (9, n))
    da = dev(A); dt = dev(np.ascontiguousarray(table.T))
    spare = torch.zeros(4096, dtype=torch.float64, device="cuda"); torch.cuda.synchronize()
    tr = rts.Tracer(8, 1)
    ep = L.RtsEigParams(); ep.n, ep.device_cov = n, da.data_ptr()
    assert lib.rts_cube_eig(tr.h, C.byref(ep), None, None) == L.RTS_ERR_INVALID and b"no cube" in lib.rts_last_error()
    tr.cube_attach(n, 2, 8, 0.0, 1.0)
    eig = lambda p, dv=None, dx=None: lib.rts_cube_eig(tr.h, C.byref(p) if p is not None else None, dv, dx)
    ep0 = L.RtsEigParams()
    assert eig(ep0) == L.RTS_ERR_INVALID and b"no covariance" in lib.rts_last_error()       # neither device_cov nor a library-owned covariance
    assert eig(ep) == L.RTS_OK
    tr._eig_n = n
    values, vectors = tr.eigenpairs()
    sp = L.RtsDoaScanParams()
    g = np.ones(n)
    sp.n, sp.first_vector, sp.m, sp.flags, sp.n_dirs, sp.g, sp.device_steering = 0, 0, n, 0, 9, g.ctypes.data, dt.data_ptr()
    scan = lambda p, out=None: lib.rts_cube_doa_scan(tr.h, C.byref(p) if p is not None else None, out)
    assert scan(sp) == L.RTS_OK
    tr._doa_n = 9
    spectrum = tr.doa_spectrum()
    assert np.array_equal(bits(spectrum), bits(rts.doa_scan_eval(vectors, g, table)))

    def changed(proto, **kw):
        q = type(proto)(); C.memmove(C.byref(q), C.byref(proto), C.sizeof(proto))
        for k, v in kw.items():
            if k.startswith("reserved_"):
                q.reserved[int(k[-1])] = v
            else:
                setattr(q, k, v)
        return q

    base = spare.data_ptr()
    bad_eig = [(None, None, None), (changed(ep, reserved0=1), None, None), (changed(ep, reserved_0=1), None, None), (changed(ep, reserved_1=1), None, None),
               (changed(ep, device_cov=da.data_ptr() + 8), None, None), (changed(ep, n=0), None, None), (changed(ep, n=D.MAX_N + 1), None, None),
               (changed(ep0, n=n + 1), None, None),
               (ep, base, None), (ep, None, base), (ep, base + 4, base + 1024), (ep, base, base + 1024 + 8),
               (ep, base, base + 16), (ep, da.data_ptr(), base), (ep, base, da.data_ptr() + 16 * n * n - 16)]
    tr.cube_covariance(fetch=False)                                                 # (a library-owned covariance of order 4, for ep0's n)
    for p, dv, dx in bad_eig:
        assert eig(p, dv, dx) == L.RTS_ERR_INVALID, lib.rts_last_error()
    nan_g = np.array([1.0, np.nan, 1.0, 1.0]); inf_g = np.array([np.inf, 1.0, 1.0, 1.0])
    bad_scan = [(None, None), (changed(sp, reserved_0=1), None), (changed(sp, reserved_1=1), None), (changed(sp, n=n + 1), None), (changed(sp, flags=2), None),
                (changed(sp, m=0), None), (changed(sp, m=n + 1), None), (changed(sp, first_vector=1), None), (changed(sp, first_vector=n + 1, m=1), None),
                (changed(sp, n_dirs=0), None), (changed(sp, n_dirs=(2 ** 31 - 1) * WG + 1), None), (changed(sp, g=None), None),
                (changed(sp, g=nan_g.ctypes.data), None), (changed(sp, g=inf_g.ctypes.data), None), (changed(sp, device_steering=None), None),
                (changed(sp, device_steering=dt.data_ptr() + 8), None), (changed(sp, device_vectors=da.data_ptr() + 8, n=n), None),
                (changed(sp, device_vectors=da.data_ptr(), n=0), None), (changed(sp, device_vectors=da.data_ptr(), n=D.MAX_N + 1), None),
                (sp, base + 4), (sp, dt.data_ptr()), (sp, dt.data_ptr() + 16 * n * 9 - 8), (changed(sp, device_vectors=da.data_ptr(), n=n), da.data_ptr() + 8)]
    for p, out in bad_scan:
        assert scan(p, out) == L.RTS_ERR_INVALID, lib.rts_last_error()
    # a refused call leaves the handle's previous products as they were
    again = tr.eigenpairs()
    assert np.array_equal(bits(again[0]), bits(values)) and np.array_equal(bits(again[1]), bits(vectors)) and np.array_equal(bits(tr.doa_spectrum()), bits(spectrum))
    small = np.zeros(2 * n * n)
    assert lib.rts_cube_eig_get(tr.h, small.ctypes.data, None, n - 1, 0) == L.RTS_ERR_CAPACITY
    assert lib.rts_cube_eig_get(tr.h, None, small.ctypes.data, 0, 2 * n * n - 1) == L.RTS_ERR_CAPACITY
    assert lib.rts_cube_eig_get(tr.h, None, None, n, 2 * n * n) == L.RTS_ERR_INVALID
    assert lib.rts_cube_eig_get(tr.h, small.ctypes.data, None, n, 0) == L.RTS_OK and np.array_equal(small[:n], values)      # either output alone
    assert lib.rts_cube_doa_get(tr.h, small.ctypes.data, 8) == L.RTS_ERR_CAPACITY and lib.rts_cube_doa_get(tr.h, None, 9) == L.RTS_ERR_INVALID
    # the products end at rts_cube_attach
    tr.cube_attach(n, 2, 8, 0.0, 1.0)
    assert lib.rts_cube_eig_get(tr.h, small.ctypes.data, None, n, 0) == L.RTS_ERR_INVALID and b"no library-owned eigenpairs" in lib.rts_last_error()
    assert lib.rts_cube_doa_get(tr.h, small.ctypes.data, 9) == L.RTS_ERR_INVALID and b"no library-owned spectrum" in lib.rts_last_error()
    assert scan(sp) == L.RTS_ERR_INVALID and b"no eigenvectors" in lib.rts_last_error()
    assert eig(ep0) == L.RTS_ERR_INVALID and b"no covariance" in lib.rts_last_error()
    assert eig(ep) == L.RTS_OK and scan(sp) == L.RTS_OK                            # and the handle goes on working
    assert np.array_equal(bits(tr.doa_spectrum()), bits(spectrum))
    tr.close()
