"""Thin Python harness over the C-ABI (tests and bench.py drive the product through this).

Nothing here computes: every method marshals numpy arrays into one call of librts_amd.so.
The production caller is C++ (include/rts_adapter.hpp, rs::RTS); see INTEGRATION.md.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import PRD_DTYPE, RESPONSE_DTYPE, GROUP_DTYPE, check, ptr


# ------------------------------------------------------------------------------- host scene helpers
def rect_mesh(w, h, d, yaw=0.0, pitch=0.0, roll=0.0):
    v = np.zeros((8, 3)); t = np.zeros((12, 3), np.uint32); n = np.zeros((12, 3))
    check(L.lib().rts_rect_mesh(w, h, d, yaw, pitch, roll, ptr(v), ptr(t), ptr(n)))
    return v, t, n


def sphere_mesh(subdivisions, radius, yaw=0.0, pitch=0.0, roll=0.0):
    nv = C.c_uint32(); nt = C.c_uint32()
    check(L.lib().rts_sphere_mesh(subdivisions, radius, yaw, pitch, roll, None, C.byref(nv), None, C.byref(nt), None))
    v = np.zeros((nv.value, 3)); t = np.zeros((nt.value, 3), np.uint32); n = np.zeros((nv.value, 3))
    check(L.lib().rts_sphere_mesh(subdivisions, radius, yaw, pitch, roll, ptr(v), C.byref(nv), ptr(t), C.byref(nt), ptr(n)))
    return v, t, n


def file_mesh(v_file, n_file, yaw=0.0, pitch=0.0, roll=0.0):
    nt = C.c_uint32(0)
    check(L.lib().rts_file_mesh(v_file.encode(), n_file.encode(), yaw, pitch, roll, None, None, None, C.byref(nt)))
    v = np.zeros((3 * nt.value, 3)); t = np.zeros((nt.value, 3), np.uint32); n = np.zeros((3 * nt.value, 3))
    check(L.lib().rts_file_mesh(v_file.encode(), n_file.encode(), yaw, pitch, roll, ptr(v), ptr(t), ptr(n), C.byref(nt)))
    return v, t, n


def vertex_rotation(verts, yaw, pitch, roll):
    v = np.ascontiguousarray(verts, np.float64).copy()
    check(L.lib().rts_vertex_rotation(ptr(v), v.shape[0], yaw, pitch, roll))
    return v


def rotation_matrix(yaw, pitch, roll):
    r = np.zeros(9)
    check(L.lib().rts_rotation_matrix(yaw, pitch, roll, ptr(r)))
    return r


def rx_sphere(pos, az, el, radius, theta_span, phi_span):
    out = L.RtsReceiverSphere(); p = np.ascontiguousarray(pos, np.float64)
    check(L.lib().rts_rx_sphere(ptr(p), az, el, radius, theta_span, phi_span, C.byref(out)))
    return dict(centre=np.array(out.centre[:]), radius=out.radius, minTheta=out.min_theta, maxTheta=out.max_theta,
                minPhi=out.min_phi, maxPhi=out.max_phi)


def merge_groups(groups, depth):
    g = np.ascontiguousarray(groups, GROUP_DTYPE)
    out = np.zeros(max(len(g), 1), GROUP_DTYPE); n = C.c_uint32(len(out))
    check(L.lib().rts_merge_groups(ptr(g), len(g), depth, ptr(out), C.byref(n)))
    return out[:n.value].copy()


def groups_to_responses(groups):
    g = np.ascontiguousarray(groups, GROUP_DTYPE)
    out = np.zeros(max(len(g), 1), RESPONSE_DTYPE); n = C.c_uint32(0)
    check(L.lib().rts_groups_to_responses(ptr(g), len(g), ptr(out), len(out), C.byref(n)))
    return out[:n.value].copy()


def kernel_wrapper(rx_results, rx_intersects, cspeed, carrier, ray_total, max_threads=1024, max_blocks=65535):
    """rs::kernel_wrapper with the caller-side pre-fill of ray_tracer.cpp:1266-1271."""
    R = rx_results.shape[0]; D = rx_intersects.shape[1] if rx_intersects.ndim == 2 else 0
    res = np.ascontiguousarray(rx_results, PRD_DTYPE).copy()
    paths = np.ascontiguousarray(rx_intersects, np.int32)
    npath = np.zeros(R); power = np.zeros(R); dop = np.zeros(R); delay = np.zeros(R); phase = np.zeros(R)
    pm = np.full(R, ray_total + 1, np.int32)
    check(L.lib().rts_kernel_wrapper(ptr(res), ptr(paths), R, D, max_threads, max_blocks, cspeed, carrier, ptr(npath),
                                     ptr(power), ptr(dop), ptr(delay), ptr(phase), ptr(pm)))
    return dict(results=res, delay=delay, phase=phase, pathMatch=pm)


INTERLEAVE_LIST = 0xffffffff


def deal_tiles(records, total_rays, tile, parts):
    """rts_deal_tiles (host code): plan tiles of `tile` launch indices, longest first, each to the worker with the least cost so far.
    Returns (part_of_tile uint32[ceil(total_rays / tile)], cost_of_part uint64[parts])."""
    r = np.ascontiguousarray(records, np.uint32)
    part = np.zeros((total_rays + tile - 1) // tile, np.uint32); cost = np.zeros(parts, np.uint64)
    check(L.lib().rts_deal_tiles(ptr(r), r.shape[0], total_rays, tile, parts, ptr(part), ptr(cost)))
    return part, cost


def build_hierarchy_host(verts, tris, split_budget=2.0):
    """rts_build_hierarchy_host: the host SAH builder on one mesh (no device): (nodes [n][32] f32 view, leaf_prim, root)"""
    v = np.ascontiguousarray(verts, np.float64); t = np.ascontiguousarray(tris, np.uint32)
    nn = C.c_uint32(0); nl = C.c_uint32(0); root = C.c_int32(-1)
    check(L.lib().rts_build_hierarchy_host(ptr(v), ptr(t), t.shape[0], split_budget, None, 0, None, 0, C.byref(nn), C.byref(nl), C.byref(root)))
    nodes = np.zeros((max(nn.value, 1), 32), np.float32); leaf = np.zeros(max(nl.value, 1), np.uint32)
    check(L.lib().rts_build_hierarchy_host(ptr(v), ptr(t), t.shape[0], split_budget, ptr(nodes), nodes.shape[0], ptr(leaf), leaf.shape[0], C.byref(nn), C.byref(nl), C.byref(root)))
    return nodes[:nn.value], leaf[:nl.value], root.value


# ------------------------------------------------------------------------------- tabulated gain / RCS patterns
class Pattern:
    """A tabulated antenna gain or RCS pattern over two angles (u, v) -- include/rts_amd.h: RtsPattern for the semantics.
    Holds its own copies of the tables; desc() is the C descriptor that points into them."""

    def __init__(self, kind, scale=1.0, flags=0, n_u=0, n_v=0, us=None, uy=None, vs=None, vy=None, grid=None, u0=0.0, du=0.0, v0=0.0, dv=0.0):
        self.kind, self.scale, self.flags, self.n_u, self.n_v = kind, float(scale), flags, n_u, n_v
        self.us, self.uy, self.vs, self.vy, self.grid_values = us, uy, vs, vy, grid
        self.u0, self.du, self.v0, self.dv = float(u0), float(du), float(v0), float(dv)

    @classmethod
    def constant(cls, v):
        return cls(L.RTS_PATTERN_CONSTANT, scale=v)

    @classmethod
    def separable(cls, u_samples, u_values, v_samples, v_values, scale=1.0, abs_u=False, abs_v=False):
        """scale * Lu(u') * Lv(v'): piecewise-linear in each angle, clamped outside the samples; u' = |u| with abs_u (v' likewise)"""
        a = [np.ascontiguousarray(x, np.float64).ravel() for x in (u_samples, u_values, v_samples, v_values)]
        if len(a[0]) != len(a[1]) or len(a[2]) != len(a[3]):
            raise ValueError("Pattern.separable: samples and values differ in length")
        flags = (L.RTS_PATTERN_ABS_U if abs_u else 0) | (L.RTS_PATTERN_ABS_V if abs_v else 0)
        return cls(L.RTS_PATTERN_SEPARABLE, scale, flags, len(a[0]), len(a[2]), *a)

    @classmethod
    def grid(cls, values, u0, du, v0, dv, scale=1.0):
        """scale * bilinear(values, u, v): values[j][i] at (u0 + i du, v0 + j dv), coordinates clamped to the grid"""
        g = np.ascontiguousarray(values, np.float64)
        if g.ndim != 2:
            raise ValueError("Pattern.grid: values must be [n_v][n_u]")
        return cls(L.RTS_PATTERN_GRID, scale, 0, g.shape[1], g.shape[0], grid=g, u0=u0, du=du, v0=v0, dv=dv)

    def desc(self):
        d = L.RtsPattern()
        d.kind, d.flags, d.n_u, d.n_v, d.scale = self.kind, self.flags, self.n_u, self.n_v, self.scale
        d.u_samples, d.u_values, d.v_samples, d.v_values, d.grid = [ptr(x) for x in (self.us, self.uy, self.vs, self.vy, self.grid_values)]
        d.u0, d.du, d.v0, d.dv = self.u0, self.du, self.v0, self.dv
        return d


def _pattern_desc(p):
    return p if isinstance(p, L.RtsPattern) else p.desc()


def pattern_eval(pattern, u, v):
    """rts_pattern_eval (pure host): the pattern's value at the points (u, v) (broadcast); raises RtsError on a malformed pattern"""
    u, v = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64))
    shape = u.shape
    u = np.ascontiguousarray(u).ravel(); v = np.ascontiguousarray(v).ravel()
    out = np.zeros(len(u))
    check(L.lib().rts_pattern_eval(C.byref(_pattern_desc(pattern)), ptr(u), ptr(v), len(u), ptr(out)))
    return out.reshape(shape)


# ------------------------------------------------------------------------------- transmit waveform (render, range compression)
class Waveform:
    """A transmit waveform: complex baseband samples at the cube's sample interval and an interpolation length (taps: 1
    sample-and-hold, or even in [2, 64] windowed sinc) -- include/rts_amd.h: RtsWaveform.  Holds its own copy of the samples."""

    def __init__(self, samples, taps=1):
        z = np.asarray(samples, np.complex128).ravel()
        self.samples = z
        self._iq = np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))
        self.taps = int(taps)

    @classmethod
    def lfm(cls, n, bandwidth_times_dt, taps=16):
        """linear FM chirp of n samples sweeping bandwidth_times_dt cycles per sample, centred on 0:
        s[m] = exp(j pi b (m - (n - 1) / 2)^2 / n)"""
        m = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
        return cls(np.exp(1j * np.pi * float(bandwidth_times_dt) * m * m / n), taps)

    @classmethod
    def coded(cls, chips, samples_per_chip=1, taps=16):
        """phase-coded waveform: every chip (a complex value: +1 / -1 of a binary code, a polyphase code's phasors) held for
        samples_per_chip samples -- the waveforms of a coded MIMO set (cube_bank) are the rows of one code family"""
        c = np.asarray(chips, np.complex128).ravel()
        if int(samples_per_chip) < 1:
            raise ValueError("Waveform.coded: samples_per_chip = %d" % samples_per_chip)
        return cls(np.repeat(c, int(samples_per_chip)), taps)

    def desc(self):
        d = L.RtsWaveform()
        d.samples, d.n_samples, d.taps = ptr(self._iq), len(self.samples), self.taps
        return d


def _waveform_desc(w):
    return w if isinstance(w, L.RtsWaveform) else w.desc()


def waveform_eval(w, x):
    """rts_waveform_eval (pure host): the waveform's continuous envelope s(x) at positions x (in samples), complex"""
    x = np.asarray(x, np.float64)
    shape = x.shape
    x = np.ascontiguousarray(x).ravel()
    out = np.zeros((len(x), 2))
    check(L.lib().rts_waveform_eval(C.byref(_waveform_desc(w)), ptr(x), len(x), ptr(out)))
    return (out[:, 0] + 1j * out[:, 1]).reshape(shape)


# ------------------------------------------------------------------------------- receiver noise (rts_noise.h)
def noise_eval(seed, index, noise_power):
    """rts_noise_eval (pure host): the receiver-noise sample of each flat cube index under seed, complex, E|n|^2 = noise_power"""
    idx = np.asarray(index, np.uint64)
    shape = idx.shape
    idx = np.ascontiguousarray(idx).ravel()
    out = np.zeros((len(idx), 2))
    check(L.lib().rts_noise_eval(int(seed), ptr(idx), len(idx), float(noise_power), ptr(out)))
    return (out[:, 0] + 1j * out[:, 1]).reshape(shape)


# ------------------------------------------------------------------------------- clutter and jammer sources (rts_source.h)
def _source_params(spatial, power, doppler, rho, range_profile, seed, n_rx, n_bins):
    """RtsSourceParams and the arrays it points to (keep them alive for the call)"""
    sp = np.ascontiguousarray(np.asarray(spatial, np.complex128))
    if sp.ndim != 2 or sp.shape[1] != n_rx:
        raise ValueError("sources: spatial of shape %s for %d receivers ([n_patches][n_rx])" % (sp.shape, n_rx))
    K = sp.shape[0]
    keep = [sp]
    p = L.RtsSourceParams()
    p.n_patches, p.seed = K, int(seed)
    p.spatial = ptr(sp.view(np.float64))
    for name, value, n in (("power", power, K), ("doppler", doppler, K), ("rho", rho, K), ("range_profile", range_profile, n_bins)):
        if value is None:
            if name in ("power", "doppler"):
                raise ValueError("sources: %s is required" % name)
            continue
        v = np.ascontiguousarray(np.asarray(value, np.float64).ravel())
        if len(v) != n:
            raise ValueError("sources: %s of %d values (%d expected)" % (name, len(v), n))
        keep.append(v)
        setattr(p, name, ptr(v))
    return p, keep


def sources_eval(cube, spatial, power, doppler, rho=None, range_profile=None, seed=0):
    """rts_sources_eval (pure host): K independent first-order Gaussian patches added to a copy of the host array cube
    [n_rx][n_pulses][n_bins] (complex), which is returned.  spatial [K][n_rx] is each patch's response on the receivers (a far-field
    patch: its steering() row), power [K] its mean power, doppler [K] in cycles per pulse, rho [K] in [0, 1] its pulse-to-pulse
    correlation (None: 1; 1 is ground clutter, a little below 1 clutter with internal motion, 0 a noise jammer), range_profile
    [n_bins] >= 0 scales the power per bin (None: 1)"""
    out = np.array(cube, np.complex128, order="C", copy=True)
    n_rx, n_pulses, nb = out.shape
    q = L.RtsCubeParams(n_rx, n_pulses, nb, 0, 0.0, 1.0)
    p, keep = _source_params(spatial, power, doppler, rho, range_profile, seed, n_rx, nb)
    check(L.lib().rts_sources_eval(C.byref(q), C.byref(p), ptr(out.view(np.float64))))
    return out


# ------------------------------------------------------------------------------- ordered-statistic CFAR (rts_cfar_os.h)
def cfar_os_n0(guard, train):
    """training cells of a full window: guard and train are (range, Doppler) cells on each side"""
    (gr, gd), (tr, td) = (int(g) for g in guard), (int(t) for t in train)
    return (2 * (gr + tr) + 1) * (2 * (gd + td) + 1) - (2 * gr + 1) * (2 * gd + 1)


def cfar_os_alpha(n, k, pfa):
    """rts_cfar_os_alpha (pure host): the threshold factor of the k-th smallest of n training cells at false-alarm rate pfa"""
    a = C.c_double(0.0)
    check(L.lib().rts_cfar_os_alpha(int(n), int(k), float(pfa), C.byref(a)))
    return a.value


def _cfar_params(p, guard, train, pfa, alpha, local_max, pri, max_detections):
    """the fields RtsCfarParams and RtsCfarOsParams share, into p"""
    p.guard_range, p.guard_doppler = (int(g) for g in guard)
    p.train_range, p.train_doppler = (int(t) for t in train)
    p.flags = L.RTS_CFAR_LOCAL_MAX if local_max else 0
    p.pfa = 0.0 if pfa is None else float(pfa)
    p.alpha = 0.0 if alpha is None else float(alpha)
    p.pri, p.max_detections = float(pri), int(max_detections)
    return p


def _cfar_os_params(guard, train, rank, pfa, alpha, local_max, pri, max_detections):
    """RtsCfarOsParams; rank None: three quarters of a full window, (3 N0) // 4"""
    p = _cfar_params(L.RtsCfarOsParams(), guard, train, pfa, alpha, local_max, pri, max_detections)
    p.rank = (3 * cfar_os_n0(guard, train)) // 4 if rank is None else int(rank)
    return p


def cfar_os_eval(map, guard=(2, 2), train=(8, 4), rank=None, pfa=None, alpha=None, local_max=True, pri=0.0, t0=0.0, dt=1.0):
    """rts_cfar_os_eval (pure host): OS-CFAR on a host map [n_rx][n_doppler][n_bins] (complex); a DETECTION_DTYPE array in flat
    (rx, doppler_bin, range_bin) order"""
    m = np.ascontiguousarray(np.asarray(map, np.complex128))
    n_rx, nd, nb = m.shape
    q = L.RtsCubeParams(n_rx, 1, nb, 0, float(t0), float(dt))
    p = _cfar_os_params(guard, train, rank, pfa, alpha, local_max, pri, 0)
    n = C.c_uint32(0)
    out = np.zeros(min(m.size, 65536), L.DETECTION_DTYPE)
    rc = L.lib().rts_cfar_os_eval(C.byref(q), ptr(m.view(np.float64)), nd, C.byref(p), ptr(out), len(out), C.byref(n))
    if rc == L.RTS_ERR_CAPACITY:
        out = np.zeros(n.value, L.DETECTION_DTYPE)
        rc = L.lib().rts_cfar_os_eval(C.byref(q), ptr(m.view(np.float64)), nd, C.byref(p), ptr(out), len(out), C.byref(n))
    check(rc)
    return out[:n.value].copy()


# ------------------------------------------------------------------------------- plot extraction (rts_plot.h)
def _plot_params(link, min_cells, pri, max_plots=0, device_list=None, n_list=0, n_doppler=0):
    """RtsPlotParams; link is the adjacency's reach (range, Doppler) in cells"""
    p = L.RtsPlotParams()
    p.link_range, p.link_doppler = (int(x) for x in link)
    p.min_cells, p.max_plots, p.pri = int(min_cells), int(max_plots), float(pri)
    p.device_list = C.c_void_p(device_list) if device_list else None
    p.n_list, p.n_doppler = int(n_list), int(n_doppler)
    return p


def plots_eval(detections, n_doppler, link=(1, 1), min_cells=1, pri=0.0, t0=0.0, dt=1.0, n_rx=None, n_bins=None):
    """rts_plots_eval (pure host): the plots of a DETECTION_DTYPE list in flat (rx, doppler_bin, range_bin) order on a map of
    n_rx x n_doppler x n_bins cells (n_rx, n_bins None: the smallest map that holds the list); a PLOT_DTYPE array in ascending
    first_index"""
    d = np.ascontiguousarray(np.asarray(detections, L.DETECTION_DTYPE))
    if n_rx is None:
        n_rx = int(d["rx"].max()) + 1 if len(d) else 1
    if n_bins is None:
        n_bins = int(d["range_bin"].max()) + 1 if len(d) else 1
    q = L.RtsCubeParams(int(n_rx), 1, int(n_bins), 0, float(t0), float(dt))
    p = _plot_params(link, min_cells, pri)
    n = C.c_uint32(0)
    out = np.zeros(max(len(d), 1), L.PLOT_DTYPE)
    check(L.lib().rts_plots_eval(C.byref(q), ptr(d) if len(d) else None, len(d), int(n_doppler), C.byref(p), ptr(out), len(out), C.byref(n)))
    return out[:n.value].copy()


# ------------------------------------------------------------------------------- tracking (rts_track.h)
def _track_params(gate, sigma, q, delay_rate_per_hz, doppler_period, confirm_hits, max_misses, tentative_misses, max_candidates, max_tracks=0,
                  device_plots=None, n_plots=0):
    """RtsTrackParams; sigma is the measurement standard deviation (delay in s, Doppler in Hz)"""
    p = L.RtsTrackParams()
    p.gate, p.q, p.delay_rate_per_hz, p.doppler_period = float(gate), float(q), float(delay_rate_per_hz), float(doppler_period)
    p.sigma_delay, p.sigma_doppler = (float(x) for x in sigma)
    p.confirm_hits, p.max_misses, p.tentative_misses = int(confirm_hits), int(max_misses), int(tentative_misses)
    p.max_candidates, p.max_tracks, p.n_plots = int(max_candidates), int(max_tracks), int(n_plots)
    p.device_plots = C.c_void_p(device_plots) if device_plots else None
    return p


def tracks_eval(tracks, next_id, T, plots, sigma, gate=9.21, q=0.0, delay_rate_per_hz=0.0, doppler_period=0.0, confirm_hits=3, max_misses=3,
                tentative_misses=0, max_candidates=L.RTS_TRACK_MAX_CAND, max_tracks=0):
    """rts_tracks_eval (pure host): one tracker step as a function -- the TRACK_DTYPE table `tracks` carried over the interval T and
    associated with the PLOT_DTYPE list `plots` (rx non-decreasing).  Returns (the stored tracks, next_id): survivors in their order,
    then the new tracks in ascending plot index; a full table (max_tracks) keeps the prefix."""
    t = np.ascontiguousarray(np.asarray(tracks, L.TRACK_DTYPE))
    z = np.ascontiguousarray(np.asarray(plots, L.PLOT_DTYPE))
    p = _track_params(gate, sigma, q, delay_rate_per_hz, doppler_period, confirm_hits, max_misses, tentative_misses, max_candidates, max_tracks)
    out = np.zeros(max(len(t) + len(z), 1), L.TRACK_DTYPE)
    n, nid = C.c_uint32(0), C.c_uint64(0)
    rc = L.lib().rts_tracks_eval(C.byref(p), ptr(t) if len(t) else None, len(t), int(next_id), float(T), ptr(z) if len(z) else None, len(z),
                                 ptr(out), len(out), C.byref(n), C.byref(nid))
    if rc != L.RTS_ERR_CAPACITY:
        check(rc)
    return out[:min(n.value, max_tracks or L.RTS_TRACK_DEFAULT_TRACKS)].copy(), nid.value


# ------------------------------------------------------------------------------- multistatic localisation (rts_locate.h)
_LOCATE_SOURCES = {"plots": (L.RTS_LOCATE_FROM_PLOTS, L.PLOT_DTYPE), "tracks": (L.RTS_LOCATE_FROM_TRACKS, L.TRACK_DTYPE),
                   "candidates": (L.RTS_LOCATE_FROM_CANDIDATES, L.TARGET_DTYPE)}


def _locate_params(tx, rx_positions, cspeed, carrier, sigma, gate, assoc_delay, box, anchors, min_receivers, n_iters, max_candidates=0, max_targets=0,
                   source="plots", device_list=None, n_list=0):
    """(RtsLocateParams, the receiver array it points to -- keep it alive for the call); sigma is the measurement standard deviation
    (delay in s, Doppler in Hz), box = (lo, hi), min_receivers None: every receiver"""
    rx = np.ascontiguousarray(np.asarray(rx_positions, np.float64).reshape(-1, 3))
    p = L.RtsLocateParams()
    p.tx[:] = [float(x) for x in tx]
    p.rx_positions = rx.ctypes.data
    p.n_rx = len(rx)
    p.anchors[:] = [int(a) for a in anchors]
    p.cspeed, p.carrier, p.gate, p.assoc_delay = float(cspeed), float(carrier), float(gate), float(assoc_delay)
    p.sigma_delay, p.sigma_doppler = (float(x) for x in sigma)
    p.box_lo[:] = [float(x) for x in box[0]]
    p.box_hi[:] = [float(x) for x in box[1]]
    p.min_receivers = len(rx) if min_receivers is None else int(min_receivers)
    p.n_iters, p.max_candidates, p.max_targets = int(n_iters), int(max_candidates), int(max_targets)
    p.source = _LOCATE_SOURCES[source][0]
    p.device_list = C.c_void_p(device_list) if device_list else None
    p.n_list = int(n_list)
    return p, rx


def locate_eval(list, tx, rx_positions, cspeed, carrier, sigma, gate=9.21, assoc_delay=1e-7, box=((-1e6,) * 3, (1e6,) * 3), anchors=(0, 1, 2), min_receivers=None,
                n_iters=4, max_candidates=0, max_targets=0, source="plots"):
    """rts_locate_eval (pure host): the targets of one frame of per-receiver records -- a PLOT_DTYPE list (rx non-decreasing), a
    TRACK_DTYPE table or, for the resolution alone, a TARGET_DTYPE list of accepted candidates -- seen from a transmitter at tx by
    the receivers at rx_positions [n_rx][3].  Returns the stored TARGET_DTYPE records in ascending candidate index (a truncated list
    gives its stored prefix)."""
    z = np.ascontiguousarray(np.asarray(list, _LOCATE_SOURCES[source][1]))
    p, keep = _locate_params(tx, rx_positions, cspeed, carrier, sigma, gate, assoc_delay, box, anchors, min_receivers, n_iters, max_candidates, max_targets, source)
    n = C.c_uint32(0)
    rc = L.lib().rts_locate_eval(C.byref(p), ptr(z) if len(z) else None, len(z), None, 0, C.byref(n))
    if rc not in (L.RTS_OK, L.RTS_ERR_CAPACITY):
        check(rc)
    out = np.zeros(max(n.value, 1), L.TARGET_DTYPE)
    rc = L.lib().rts_locate_eval(C.byref(p), ptr(z) if len(z) else None, len(z), ptr(out), len(out), C.byref(n))
    if rc != L.RTS_ERR_CAPACITY:
        check(rc)
    return out[:min(n.value, max_targets or L.RTS_LOCATE_DEFAULT_TARGETS)].copy()


# ------------------------------------------------------------------------------- track-before-detect (rts_tbd.h)
def _tbd_params(half, depth, score, scale, decay, delay_rate_per_hz, pri):
    """RtsTbdParams; half is the transition window (Doppler, range) in cells on each side"""
    p = L.RtsTbdParams()
    p.half_doppler, p.half_range = (int(x) for x in half)
    p.depth = int(depth)
    p.score = {"power": L.RTS_TBD_POWER, "amplitude": L.RTS_TBD_AMPLITUDE}.get(score, score)
    p.scale, p.decay, p.delay_rate_per_hz, p.pri = float(scale), float(decay), float(delay_rate_per_hz), float(pri)
    return p


def _tbd_extract_params(threshold, local_max, max_tracks, pri):
    e = L.RtsTbdExtractParams()
    e.threshold, e.pri, e.max_tracks = float(threshold), float(pri), int(max_tracks)
    e.flags = L.RTS_TBD_LOCAL_MAX if local_max else 0
    return e


def tbd_step_eval(map, merit_in, T, half=(1, 2), depth=8, score="power", scale=1.0, decay=1.0, delay_rate_per_hz=0.0, pri=0.0, dt=1.0):
    """rts_tbd_step_eval (pure host): one track-before-detect step on a host map [n_rx][n_doppler][n_bins] (complex) from the merit
    map merit_in (None: the first frame).  Returns (merit f64, pointers uint8, both of the map's shape, shifts int32 [n_doppler])."""
    m = np.ascontiguousarray(np.asarray(map, np.complex128))
    n_rx, nd, nb = m.shape
    q = L.RtsCubeParams(n_rx, 1, nb, 0, 0.0, float(dt))
    p = _tbd_params(half, depth, score, scale, decay, delay_rate_per_hz, pri)
    prev = None if merit_in is None else np.ascontiguousarray(np.asarray(merit_in, np.float64).reshape(m.shape))
    merit, code, shifts = np.zeros(m.shape), np.zeros(m.shape, np.uint8), np.zeros(nd, np.int32)
    check(L.lib().rts_tbd_step_eval(C.byref(q), ptr(m.view(np.float64)), nd, ptr(prev), C.byref(p), float(T), ptr(merit), ptr(code), ptr(shifts)))
    return merit, code, shifts


def tbd_extract_eval(merit, ptrs, shifts, threshold, half=(1, 2), depth=8, local_max=True, max_tracks=0, pri=0.0, t0=0.0, dt=1.0):
    """rts_tbd_extract_eval (pure host): the candidates of the merit map [n_rx][n_doppler][n_bins] walked back through the pointer
    maps ptrs [n_frames][n_rx][n_doppler][n_bins] and shift tables shifts [n_frames][n_doppler], oldest first.  Returns (the stored
    TBD_TRACK_DTYPE records, their paths uint32 [n][depth][2])."""
    m = np.ascontiguousarray(np.asarray(merit, np.float64))
    n_rx, nd, nb = m.shape
    c = np.ascontiguousarray(np.asarray(ptrs, np.uint8)); s = np.ascontiguousarray(np.asarray(shifts, np.int32))
    n_frames = len(c)
    assert c.shape == (n_frames,) + m.shape and s.shape == (n_frames, nd)
    q = L.RtsCubeParams(n_rx, 1, nb, 0, float(t0), float(dt))
    p = _tbd_params(half, depth, "power", 1.0, 1.0, 0.0, 0.0)
    e = _tbd_extract_params(threshold, local_max, max_tracks, pri)
    n = C.c_uint32(0)
    cap = min(m.size, max_tracks or L.RTS_TBD_MAX_TRACKS)
    out = np.zeros(max(cap, 1), L.TBD_TRACK_DTYPE); paths = np.zeros((max(cap, 1), int(depth), 2), np.uint32)
    rc = L.lib().rts_tbd_extract_eval(C.byref(q), nd, C.byref(p), ptr(m), ptr(c), ptr(s), n_frames, C.byref(e), ptr(out), ptr(paths), cap, C.byref(n))
    if rc != L.RTS_ERR_CAPACITY:
        check(rc)
    k = min(n.value, cap)
    return out[:k].copy(), paths[:k].copy()


# ------------------------------------------------------------------------------- backprojection imaging (rts_image.h)
def _image_params(origin, step_x, step_y, n_x, n_y, tx_positions, rx_positions, cspeed, carrier, taps, first, count, weights, accumulate, n_rx):
    """RtsImageParams and the arrays it points to (keep them alive for the call).  tx_positions [P][3]; rx_positions [n_rx][P][3]
    ([P][3] for one receiver); count None: every position given"""
    tx = np.ascontiguousarray(np.asarray(tx_positions, np.float64).reshape(-1, 3))
    P = len(tx) if count is None else int(count)
    rx = np.ascontiguousarray(np.asarray(rx_positions, np.float64).reshape(-1, 3))
    if len(tx) != P or len(rx) != n_rx * P:
        raise ValueError("backprojection: %d transmitter and %d receiver positions for %d pulses and %d receivers" % (len(tx), len(rx), P, n_rx))
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.float64).ravel())
    if w is not None and len(w) != P:
        raise ValueError("backprojection: %d weights for %d pulses" % (len(w), P))
    p = L.RtsImageParams()
    p.n_x, p.n_y, p.taps, p.flags = int(n_x), int(n_y), int(taps), L.RTS_IMAGE_ACCUMULATE if accumulate else 0
    p.first_pulse, p.n_pulses = int(first), P
    for k in range(3):
        p.origin[k], p.step_x[k], p.step_y[k] = float(origin[k]), float(step_x[k]), float(step_y[k])
    p.cspeed, p.carrier = float(cspeed), float(carrier)
    p.tx_position, p.rx_position, p.pulse_weight = ptr(tx), ptr(rx), ptr(w)
    return p, (tx, rx, w)


def backproject_eval(cube, t0, dt, origin, step_x, step_y, n_x, n_y, tx_positions, rx_positions, cspeed, carrier, taps=8, first=0, count=None,
                     weights=None, out=None):
    """rts_backproject_eval (pure host): the backprojected image of a host cube [n_rx][n_pulses][n_bins] (complex), complex
    [n_rx][n_y][n_x]; out: an image to ADD to (RTS_IMAGE_ACCUMULATE), returned updated"""
    cube = np.ascontiguousarray(np.asarray(cube, np.complex128))
    n_rx, n_p, n_bins = cube.shape
    q = L.RtsCubeParams(n_rx, n_p, n_bins, 0, float(t0), float(dt))
    p, keep = _image_params(origin, step_x, step_y, n_x, n_y, tx_positions, rx_positions, cspeed, carrier, taps, first, count, weights, out is not None, n_rx)
    img = np.zeros((n_rx, int(n_y), int(n_x)), np.complex128) if out is None else np.ascontiguousarray(np.array(out, np.complex128))
    if img.shape != (n_rx, int(n_y), int(n_x)):
        raise ValueError("backproject_eval: out has shape %s" % (img.shape,))
    check(L.lib().rts_backproject_eval(C.byref(q), ptr(cube.view(np.float64)), C.byref(p), ptr(img.view(np.float64))))
    return img


def image_frame(positions, motions):
    """ISAR change of frame: radar positions [..., P, 3] (world) -> the target's frame, p' = R_j^T (p - position_j) per pulse j.
    motions: per pulse a dict(position=, rotation= 9 values row-major or None) or an RtsTargetMotion"""
    p = np.asarray(positions, np.float64)
    out = np.empty_like(p)
    if p.shape[-2] != len(motions):
        raise ValueError("image_frame: %d pulses of positions, %d motions" % (p.shape[-2], len(motions)))
    for j, m in enumerate(motions):
        if isinstance(m, L.RtsTargetMotion):
            pos = np.array(m.position[:]); rot = np.array(m.rotation[:]).reshape(3, 3) if m.has_rotation else None
        else:
            pos = np.asarray(m["position"], np.float64); rot = m.get("rotation")
            rot = None if rot is None else np.asarray(rot, np.float64).reshape(3, 3)
        d = p[..., j, :] - pos
        out[..., j, :] = d if rot is None else d @ rot              # (R^T d)_i = sum_k R[k][i] d_k
    return out


# ------------------------------------------------------------------------------- slow-time spectrogram (rts_stft.h)
_WINDOW_KINDS = {"rect": L.RTS_WINDOW_RECT, "hann": L.RTS_WINDOW_HANN, "hamming": L.RTS_WINDOW_HAMMING, "blackman": L.RTS_WINDOW_BLACKMAN}


def window(kind, n):
    """rts_window_make (pure host): the symmetric window "rect", "hann", "hamming" or "blackman" (or an RTS_WINDOW_* value) of n points"""
    out = np.zeros(max(int(n), 1))
    check(L.lib().rts_window_make(_WINDOW_KINDS.get(kind, kind), int(n), ptr(out)))
    return out


def _stft_params(window_len, hop, n_fft, window, first, count, first_bin, n_bins, power, sum_bins, n_pulses_cube):
    """RtsStftParams and the window array it points to (keep it alive for the call); count None: to the cube's last row"""
    w = None if window is None else np.ascontiguousarray(np.asarray(window, np.float64).ravel())
    if w is not None and len(w) != int(window_len):
        raise ValueError("spectrogram: a window of %d values for window_len = %d" % (len(w), window_len))
    p = L.RtsStftParams()
    p.first_pulse, p.n_pulses = int(first), int(n_pulses_cube - first if count is None else count)
    p.window_len, p.hop, p.n_fft, p.first_bin, p.n_bins = int(window_len), int(hop), int(n_fft), int(first_bin), int(n_bins)
    p.flags = (L.RTS_STFT_POWER if power else 0) | (L.RTS_STFT_SUM_BINS if sum_bins else 0)
    p.window = ptr(w)
    return p, w


def _stft_shape(n_rx, n_frames, n_fft, n_gate, power, sum_bins):
    """(shape, dtype) of a spectrogram in the layout of include/rts_amd.h"""
    if sum_bins:
        return (n_rx, n_frames, n_fft), np.float64
    return (n_rx, n_frames, n_fft, n_gate), np.float64 if power else np.complex128


def stft_frames(n_pulses, window_len, hop):
    """the number of whole frames of a span of n_pulses pulses"""
    return 1 + (int(n_pulses) - int(window_len)) // int(hop)


def stft_eval(cube, window_len, hop, n_fft, window=None, first=0, count=None, first_bin=0, n_bins=0, power=False, sum_bins=False):
    """rts_stft_eval (pure host): the spectrogram of a host cube [n_rx][n_pulses][n_bins] (complex): complex
    [n_rx][n_frames][n_fft][n_gate], float64 of that shape with power, float64 [n_rx][n_frames][n_fft] with power and sum_bins"""
    cube = np.ascontiguousarray(np.asarray(cube, np.complex128))
    n_rx, n_p, nb = cube.shape
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, 0.0, 1.0)
    p, keep = _stft_params(window_len, hop, n_fft, window, first, count, first_bin, n_bins, power, sum_bins, n_p)
    n_gate = p.n_bins if p.n_bins else max(nb - p.first_bin, 0)
    n_frames = max(stft_frames(p.n_pulses, p.window_len, max(p.hop, 1)), 0)
    shape, dtype = _stft_shape(n_rx, n_frames, p.n_fft, n_gate, power, sum_bins)
    out = np.zeros(shape, dtype)
    nf = C.c_uint32(0)
    check(L.lib().rts_stft_eval(C.byref(q), ptr(cube.view(np.float64)), C.byref(p), ptr(out), C.byref(nf)))
    assert nf.value == n_frames
    return out


def spectrogram_axes(window_len, hop, n_fft, n_pulses, pri, first=0):
    """the axes of a spectrogram of pulses first .. first + n_pulses - 1: (the pulse index each frame is centred on, float64
    [n_frames]; the Doppler of each row in Hz, float64 [n_fft], row k at k' / (n_fft pri) with k' = k wrapped into
    [-n_fft / 2, n_fft / 2): a closing range is a positive Doppler)"""
    f = np.arange(stft_frames(n_pulses, window_len, hop), dtype=np.float64)
    centres = first + f * hop + (window_len - 1) / 2.0
    k = np.arange(n_fft)
    k = np.where(k >= n_fft // 2, k - n_fft, k).astype(np.float64)
    return centres, k / (n_fft * float(pri))


# ------------------------------------------------------------------------------- autofocus: alignment, PGA, correction (rts_focus.h)
def _gate(gate):
    """(first_bin, n_gate) of a gate given as None (the whole row) or (first_bin, n_gate); n_gate 0: to the row's last bin"""
    return (0, 0) if gate is None else (int(gate[0]), int(gate[1]))


def _align_params(first, count, gate, max_lag, n_iters, integer, n_pulses_cube):
    p = L.RtsAlignParams()
    p.first_pulse, p.n_pulses = int(first), int(n_pulses_cube - first if count is None else count)
    p.first_bin, p.n_gate = _gate(gate)
    p.max_lag, p.n_iters, p.flags = int(max_lag), int(n_iters), L.RTS_ALIGN_INTEGER if integer else 0
    return p


def _pga_params(first, count, gate, n_iters, window0, window_min, n_pulses_cube):
    p = L.RtsPgaParams()
    p.first_pulse, p.n_pulses = int(first), int(n_pulses_cube - first if count is None else count)
    p.first_bin, p.n_gate = _gate(gate)
    p.n_iters, p.window0, p.window_min = int(n_iters), int(window0), int(window_min)
    return p


def _correct_params(first, count, taps, shifts, phase, use_align, use_pga, n_rx, n_pulses_cube):
    """RtsCorrectParams and the arrays it points to (keep them alive for the call)"""
    p = L.RtsCorrectParams()
    p.first_pulse, p.n_pulses, p.taps = int(first), int(n_pulses_cube - first if count is None else count), int(taps)
    p.flags = (L.RTS_CORRECT_USE_ALIGN if use_align else 0) | (L.RTS_CORRECT_USE_PGA if use_pga else 0)
    keep = []
    for name, a in (("shifts", shifts), ("phase", phase)):
        if a is None:
            continue
        a = np.ascontiguousarray(np.asarray(a, np.float64))
        if a.size != n_rx * p.n_pulses:
            raise ValueError("correct: %s of %d values for %d receivers x %d rows" % (name, a.size, n_rx, p.n_pulses))
        setattr(p, name, ptr(a)); keep.append(a)
    return p, keep


def align_eval(cube, first=0, count=None, gate=None, max_lag=8, n_iters=4, integer=False):
    """rts_align_eval (pure host): the range shifts, float64 [n_rx][count] in bins, of a host cube [n_rx][n_pulses][n_bins] (complex)"""
    cube = np.ascontiguousarray(np.asarray(cube, np.complex128))
    n_rx, n_p, nb = cube.shape
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, 0.0, 1.0)
    p = _align_params(first, count, gate, max_lag, n_iters, integer, n_p)
    out = np.zeros((n_rx, max(min(p.n_pulses, n_p), 1)))
    check(L.lib().rts_align_eval(C.byref(q), ptr(cube.view(np.float64)), C.byref(p), ptr(out)))
    return out


def pga_eval(cube, first=0, count=None, gate=None, n_iters=6, window0=0, window_min=0):
    """rts_pga_eval (pure host): (the phase error float64 [n_rx][count] in cycles, the iterations' rms float64 [n_rx][n_iters])"""
    cube = np.ascontiguousarray(np.asarray(cube, np.complex128))
    n_rx, n_p, nb = cube.shape
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, 0.0, 1.0)
    p = _pga_params(first, count, gate, n_iters, window0, window_min, n_p)
    phase = np.zeros((n_rx, max(min(p.n_pulses, n_p), 1))); rms = np.zeros((n_rx, max(min(p.n_iters, L.RTS_PGA_MAX_ITERS), 1)))
    check(L.lib().rts_pga_eval(C.byref(q), ptr(cube.view(np.float64)), C.byref(p), ptr(phase), ptr(rms)))
    return phase, rms


def correct_eval(cube, shifts=None, phase=None, first=0, count=None, taps=8):
    """rts_correct_eval (pure host): a copy of the host cube with rows first .. first + count - 1 resampled at n + shifts (bins) and
    rotated by -phase (cycles); shifts, phase: [n_rx][count] or None"""
    out = np.array(cube, np.complex128, order="C", copy=True)
    n_rx, n_p, nb = out.shape
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, 0.0, 1.0)
    p, keep = _correct_params(first, count, taps, shifts, phase, False, False, n_rx, n_p)
    check(L.lib().rts_correct_eval(C.byref(q), ptr(out.view(np.float64)), C.byref(p)))
    return out


# ------------------------------------------------------------------------------- FMCW: beat render, range transform (rts_beat.h)
_RENDER_SOURCES = {"rays": L.RTS_RENDER_RAYS, "paths": L.RTS_RENDER_PATHS}


def _beat_params(slope, duration, source, doppler):
    p = L.RtsBeatParams()
    p.slope, p.duration = float(slope), float(duration)
    p.source, p.flags = _RENDER_SOURCES.get(source, source), L.RTS_RENDER_DOPPLER if doppler else 0
    return p


def beat_eval(cube, pulse, contributions, slope, duration, t0, dt, source="rays", doppler=True):
    """rts_beat_eval (pure host): the dechirped beat signal of the contributions -- (rx, complex amplitude, delay, Doppler) tuples, or a
    BEAT_CONTRIBUTION_DTYPE array -- added into row `pulse` of the host cube [n_rx][n_pulses][n_bins] (complex128, in place when it
    is a contiguous complex128 array); returns the cube"""
    cube = np.ascontiguousarray(np.asarray(cube, np.complex128))
    n_rx, n_p, nb = cube.shape
    if isinstance(contributions, np.ndarray) and contributions.dtype == L.BEAT_CONTRIBUTION_DTYPE:
        c = np.ascontiguousarray(contributions)
    else:
        c = np.zeros(len(contributions), L.BEAT_CONTRIBUTION_DTYPE)
        for k, (rx, a, tau, f) in enumerate(contributions):
            c[k] = (rx, 0, complex(a).real, complex(a).imag, tau, f)
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, float(t0), float(dt))
    p = _beat_params(slope, duration, source, doppler)
    check(L.lib().rts_beat_eval(C.byref(q), C.byref(p), ptr(c) if len(c) else None, len(c), int(pulse), ptr(cube.view(np.float64))))
    return cube


def _range_params(n_fft, window, first, count, first_bin, n_samples, n_out, reverse, n_pulses_cube, n_bins_cube):
    """RtsRangeParams and the window array it points to (keep it alive for the call); count None: to the cube's last row"""
    w = None if window is None else np.ascontiguousarray(np.asarray(window, np.float64).ravel())
    want = int(n_samples) if n_samples else max(n_bins_cube - int(first_bin), 0)
    if w is not None and len(w) != want:
        raise ValueError("range transform: a window of %d values for %d samples" % (len(w), want))
    p = L.RtsRangeParams()
    p.first_pulse, p.n_pulses = int(first), int(n_pulses_cube - first if count is None else count)
    p.first_bin, p.n_samples, p.n_fft, p.n_out = int(first_bin), int(n_samples), int(n_fft), int(n_out)
    p.flags = L.RTS_RANGE_REVERSE if reverse else 0
    p.window = ptr(w)
    return p, w


def range_eval(cube, n_fft, window=None, first=0, count=None, first_bin=0, n_samples=0, n_out=0, reverse=False):
    """rts_range_eval (pure host): the fast-time transform of rows first .. first + count - 1 of a host cube
    [n_rx][n_pulses][n_bins] (complex): complex [n_rx][count][n_out or n_fft]"""
    cube = np.ascontiguousarray(np.asarray(cube, np.complex128))
    n_rx, n_p, nb = cube.shape
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, 0.0, 1.0)
    p, keep = _range_params(n_fft, window, first, count, first_bin, n_samples, n_out, reverse, n_p, nb)
    out = np.zeros((n_rx, max(p.n_pulses, 0), p.n_out if p.n_out else p.n_fft), np.complex128)
    check(L.lib().rts_range_eval(C.byref(q), ptr(cube.view(np.float64)), C.byref(p), ptr(out.view(np.float64))))
    return out


def beat_axis(slope, n_fft, dt, n_out=0):
    """the range axis of a transformed beat cube: (delay of each kept bin in s, float64 [n_out or n_fft], bin k at
    k / (|slope| n_fft dt); the `reverse` flag the transform needs: True for an up-chirp, whose beat frequency -S tau is negative).
    The step delays[1] is the dt to attach the output with (t0 = 0)."""
    n = int(n_out) if n_out else int(n_fft)
    return np.arange(n, dtype=np.float64) / (abs(float(slope)) * int(n_fft) * float(dt)), slope > 0


_BEAM_SOURCES = {"cube": L.RTS_BEAM_FROM_CUBE, "map": L.RTS_BEAM_FROM_MAP, "pointer": L.RTS_BEAM_FROM_POINTER}


def steering(positions, directions, wavelength, taper=None):
    """rts_steering_make (pure host): far-field steering weights complex [n_beams][n_rx] in the cube's phase convention, for element
    centres positions [n_rx][3] (m), beam directions [n_beams][2] = (az, el) in radians and an optional real taper [n_rx];
    y = sum conj(w) z peaks in the beam steered at a plane wave's direction of arrival"""
    pos = np.ascontiguousarray(np.asarray(positions, np.float64).reshape(-1, 3))
    d = np.ascontiguousarray(np.asarray(directions, np.float64).reshape(-1, 2))
    t = None if taper is None else np.ascontiguousarray(np.asarray(taper, np.float64).ravel())
    if t is not None and len(t) != len(pos):
        raise ValueError("steering: a taper of %d values for %d receivers" % (len(t), len(pos)))
    w = np.zeros((len(d), len(pos)), np.complex128)
    check(L.lib().rts_steering_make(ptr(pos), len(pos), ptr(d), len(d), float(wavelength), ptr(t), ptr(w.view(np.float64))))
    return w


def _beam_params(weights, n_rx, source, first, count, power, peak, device_in, n_rows_in):
    """RtsBeamParams and the weight array it points to (keep it alive for the call); count None: to the source's last row"""
    w = np.ascontiguousarray(np.asarray(weights, np.complex128))
    if w.ndim != 2 or w.shape[1] != n_rx:
        raise ValueError("beamform: weights of shape %s for %d receivers ([n_beams][n_rx])" % (w.shape, n_rx))
    p = L.RtsBeamParams()
    p.n_beams, p.source = w.shape[0], _BEAM_SOURCES.get(source, source)
    p.first_row, p.n_rows, p.n_rows_in = int(first), int(count or 0), int(n_rows_in)
    p.flags = (L.RTS_BEAM_POWER if power else 0) | (L.RTS_BEAM_PEAK if peak else 0)
    p.weights = ptr(w.view(np.float64))
    p.device_in = device_in if device_in else None
    return p, w


def _beam_out(n_beams, n_rows, n_bins, power, peak):
    """the host array of a beamformer's output: (P*, coordinate) per cell, power or complex per beam"""
    n_rows = max(n_rows, 0)
    if peak:
        return np.zeros((n_rows, n_bins, 2), np.float64)
    return np.zeros((n_beams, n_rows, n_bins), np.float64 if power else np.complex128)


def beamform_eval(inp, weights, first=0, count=None, power=False, peak=False):
    """rts_beamform_eval (pure host): beams y[b] = sum_rx conj(w[b][rx]) z[rx] of rows first .. first + count - 1 (default: to the last)
    of a host array [n_rx][n_rows][n_bins] (complex): complex [n_beams][count][n_bins], its power (float64, same shape) with power,
    or float64 [count][n_bins][2] = (largest beam power, refined beam coordinate) with peak"""
    inp = np.ascontiguousarray(np.asarray(inp, np.complex128))
    n_rx, rows, nb = inp.shape
    q = L.RtsCubeParams(n_rx, rows, nb, 0, 0.0, 1.0)
    p, keep = _beam_params(weights, n_rx, "cube", first, count, power, peak, None, 0)
    out = _beam_out(p.n_beams, p.n_rows if p.n_rows else rows - p.first_row, nb, power, peak)
    check(L.lib().rts_beamform_eval(C.byref(q), ptr(inp.view(np.float64)), rows, C.byref(p), ptr(out.view(np.float64))))
    return out


def beam_angles(coordinate, directions):
    """the caller's beam directions ([n_beams] or [n_beams][k], e.g. (az, el)) interpolated linearly at the beam coordinate of a
    RTS_BEAM_PEAK output (beam index + offset): an array of coordinate's shape (with a trailing axis of k)"""
    d = np.asarray(directions, np.float64)
    c = np.asarray(coordinate, np.float64)
    idx = np.arange(len(d), dtype=np.float64)
    if d.ndim == 1:
        return np.interp(c, idx, d)
    return np.stack([np.interp(c, idx, d[:, k]) for k in range(d.shape[1])], axis=-1)


def _cov_params(source, first, count, first_bin, n_bins, skip, device_in, n_rows_in):
    """RtsCovParams: rows first .. first + count - 1 (count None: to the last), bins first_bin .. first_bin + n_bins - 1 (n_bins None: to
    the last) without skip = (first skipped bin, how many) or None"""
    p = L.RtsCovParams()
    p.source, p.n_rows_in = _BEAM_SOURCES.get(source, source), int(n_rows_in)
    p.first_row, p.n_rows, p.first_bin, p.n_bins = int(first), int(count or 0), int(first_bin), int(n_bins or 0)
    p.skip_first_bin, p.skip_n_bins = (int(skip[0]), int(skip[1])) if skip is not None else (0, 0)
    p.device_in = device_in if device_in else None
    return p


def covariance_eval(inp, first=0, count=None, first_bin=0, n_bins=None, skip=None):
    """rts_covariance_eval (pure host): the sample covariance R[i][j] = mean over the training cells of z_i conj(z_j) of a host array
    [n_rx][n_rows][n_bins] (complex) -- rows first .. first + count - 1, bins first_bin .. first_bin + n_bins - 1 without the skip
    interval (first skipped bin, how many): complex [n_rx][n_rx]"""
    inp = np.ascontiguousarray(np.asarray(inp, np.complex128))
    n_rx, rows, nb = inp.shape
    q = L.RtsCubeParams(n_rx, rows, nb, 0, 0.0, 1.0)
    p = _cov_params("cube", first, count, first_bin, n_bins, skip, None, 0)
    out = np.zeros((n_rx, n_rx), np.complex128)
    check(L.lib().rts_covariance_eval(C.byref(q), ptr(inp.view(np.float64)), rows, C.byref(p), ptr(out.view(np.float64))))
    return out


def _mvdr_params(steering, n_rx, loading, device_cov):
    """RtsMvdrParams and the steering array it points to (keep it alive for the call)"""
    s = np.ascontiguousarray(np.asarray(steering, np.complex128))
    if s.ndim != 2 or (n_rx and s.shape[1] != n_rx):
        raise ValueError("mvdr: steering of shape %s for %d receivers ([n_beams][n_rx])" % (s.shape, n_rx))
    p = L.RtsMvdrParams()
    p.n_beams, p.n_rx, p.loading = s.shape[0], s.shape[1], float(loading)
    p.steering = ptr(s.view(np.float64))
    p.device_cov = device_cov if device_cov else None
    return p, s


def mvdr_eval(cov, steering, loading=0.0):
    """rts_mvdr_eval (pure host): the MVDR weights w[b] = A^-1 s_b / (s_b^H A^-1 s_b), A = cov + loading I, of steering rows complex
    [n_beams][n_rx] (steering) by Cholesky: complex [n_beams][n_rx], a weight table of beamform_eval / cube_beamform"""
    cov = np.ascontiguousarray(np.asarray(cov, np.complex128))
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError("mvdr_eval: a covariance of shape %s ([n_rx][n_rx])" % (cov.shape,))
    p, keep = _mvdr_params(steering, cov.shape[0], loading, None)
    out = np.zeros((p.n_beams, cov.shape[0]), np.complex128)
    check(L.lib().rts_mvdr_eval(ptr(cov.view(np.float64)), cov.shape[0], C.byref(p), ptr(out.view(np.float64))))
    return out


def _rx_mask(rx):
    """RtsCancelParams.rx_mask: None (0: every receiver but the reference), an integer mask, or the receivers' indices"""
    if rx is None:
        return 0
    if isinstance(rx, (int, np.integer)):
        return int(rx)
    m = 0
    for r in rx:
        m |= 1 << int(r)
    return m


def _cancel_params(ref_rx, n_taps, first, count, rows_per_block, rx, loading, n_pulses_cube):
    p = L.RtsCancelParams()
    p.ref_rx, p.n_taps, p.first_pulse = int(ref_rx), int(n_taps), int(first)
    p.n_pulses = int(n_pulses_cube - first if count is None else count)
    p.rows_per_block, p.rx_mask, p.loading = int(rows_per_block), _rx_mask(rx), float(loading)
    return p


def _xcorr_params(ref_rx, n_lags, first_lag, first, count, n_pulses_cube):
    p = L.RtsXcorrParams()
    p.ref_rx, p.first_pulse, p.n_pulses = int(ref_rx), int(first), int(n_pulses_cube - first if count is None else count)
    p.first_lag, p.n_lags = int(first_lag), int(n_lags)
    return p


def _cancel_blocks(n_rows, rows_per_block):
    R = n_rows if rows_per_block == 0 or rows_per_block > n_rows else rows_per_block
    return (n_rows + R - 1) // R


def cancel_eval(cube, ref_rx, n_taps, rows_per_block=0, first=0, count=None, rx=None, loading=0.0):
    """rts_cancel_eval (pure host): batch ECA of a host cube [n_rx][n_pulses][n_bins] (complex) -- per block of rows_per_block rows
    (0: the whole span) of rows first .. first + count - 1 the least-squares fit of the n_taps lagged copies of receiver ref_rx's row
    is subtracted from the receivers rx (None: all but ref_rx; indices or a mask).  Returns (the cancelled cube, the coefficients
    complex [n_rx][n_blocks][n_taps], (n_blocks, n_failed))"""
    out = np.ascontiguousarray(np.array(cube, np.complex128))
    n_rx, n_p, nb = out.shape
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, 0.0, 1.0)
    p = _cancel_params(ref_rx, n_taps, first, count, rows_per_block, rx, loading, n_p)
    coeffs = np.zeros((n_rx, max(_cancel_blocks(max(p.n_pulses, 1), p.rows_per_block), 1), max(p.n_taps, 1)), np.complex128)
    nblk, nfail = C.c_uint32(0), C.c_uint32(0)
    check(L.lib().rts_cancel_eval(C.byref(q), ptr(out.view(np.float64)), C.byref(p), ptr(coeffs.view(np.float64)), C.byref(nblk), C.byref(nfail)))
    return out, coeffs, (nblk.value, nfail.value)


def xcorr_eval(cube, ref_rx, n_lags, first_lag=0, first=0, count=None):
    """rts_xcorr_eval (pure host): z[r][p][l - first_lag] = sum_n y_r[p][n + l] conj(ref[p][n]) of a host cube [n_rx][n_pulses][n_bins]
    (complex) with ref the row of receiver ref_rx, over rows first .. first + count - 1: complex [n_rx][count][n_lags]"""
    cube = np.ascontiguousarray(np.asarray(cube, np.complex128))
    n_rx, n_p, nb = cube.shape
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, 0.0, 1.0)
    p = _xcorr_params(ref_rx, n_lags, first_lag, first, count, n_p)
    out = np.zeros((n_rx, max(p.n_pulses, 1), max(p.n_lags, 1)), np.complex128)
    check(L.lib().rts_xcorr_eval(C.byref(q), ptr(cube.view(np.float64)), C.byref(p), ptr(out.view(np.float64))))
    return out


def _bank_params(waves, code, first, count, n_pulses_cube):
    """RtsBankParams and what it points to (keep it alive for the call)"""
    ws = [w for w in waves]
    descs = (L.RtsWaveform * max(len(ws), 1))()
    for i, w in enumerate(ws):
        d = _waveform_desc(w)
        descs[i].samples, descs[i].n_samples, descs[i].taps = d.samples, d.n_samples, d.taps
        descs[i].reserved[0], descs[i].reserved[1] = d.reserved[0], d.reserved[1]
    p = L.RtsBankParams()
    p.waves, p.n_waves, p.first_pulse = descs, len(ws), int(first)
    p.n_pulses = int(n_pulses_cube - first if count is None else count)
    keep = [ws, descs]
    if code is not None:
        c = np.ascontiguousarray(np.asarray(code, np.complex128))
        if c.shape != (len(ws), p.n_pulses):
            raise ValueError("bank: code of shape %s for %d waveforms x %d pulses" % (c.shape, len(ws), p.n_pulses))
        keep.append(c)
        p.code = ptr(c.view(np.float64))
    return p, keep


def bank_eval(cube, waves, code=None, first=0, count=None):
    """rts_bank_eval (pure host): the matched-filter bank of a host cube [n_rx][n_pulses][n_bins] (complex) -- every row of rows
    first .. first + count - 1 of every receiver correlated with each of the waveforms (Waveform or RtsWaveform), then multiplied by
    conj(code[t][p]) (code complex [n_waves][count], None: no multiply): complex [n_waves * n_rx][count][n_bins], virtual element
    t * n_rx + r"""
    cube = np.ascontiguousarray(np.asarray(cube, np.complex128))
    n_rx, n_p, nb = cube.shape
    q = L.RtsCubeParams(n_rx, n_p, nb, 0, 0.0, 1.0)
    p, keep = _bank_params(waves, code, first, count, n_p)
    out = np.zeros((max(p.n_waves, 1) * n_rx, max(p.n_pulses, 1), nb), np.complex128)
    check(L.lib().rts_bank_eval(C.byref(q), ptr(cube.view(np.float64)), C.byref(p), ptr(out.view(np.float64))))
    return out


def virtual_positions(tx_offsets, rx_positions):
    """the positions [n_tx * n_rx][3] of the virtual elements of a MIMO array in the bank's element order (t * n_rx + r):
    rx_positions[r] + tx_offsets[t] -- for a far target the echo of transmitter t on receiver r has the phase of one element there.
    The steering table of the virtual cube is steering(virtual_positions(...), ...)"""
    tx = np.asarray(tx_offsets, np.float64).reshape(-1, 3)
    rx = np.asarray(rx_positions, np.float64).reshape(-1, 3)
    return (tx[:, None, :] + rx[None, :, :]).reshape(-1, 3)


def eig_eval(cov, sweeps=False):
    """rts_eig_eval (pure host): the eigenpairs of a Hermitian matrix complex [n][n] (its lower triangle and the real part of its
    diagonal are read) by one-sided Jacobi: (eigenvalues float64 [n] in descending order, eigenvectors complex [n][n], ROW k the
    eigenvector of value k: a weight row of beamform_eval); with sweeps also the number of sweeps that rotated"""
    cov = np.ascontiguousarray(np.asarray(cov, np.complex128))
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1]:
        raise ValueError("eig_eval: a matrix of shape %s ([n][n])" % (cov.shape,))
    n = cov.shape[0]
    values = np.zeros(n, np.float64); vectors = np.zeros((n, n), np.complex128); ns = C.c_uint32(0)
    check(L.lib().rts_eig_eval(ptr(cov.view(np.float64)), n, ptr(values), ptr(vectors.view(np.float64)), C.byref(ns)))
    return (values, vectors, ns.value) if sweeps else (values, vectors)


def _steering_table(steering):
    """a host steering table [n_dirs][n] (steering()'s rows) as the scan reads it: element-major complex [n][n_dirs]"""
    a = np.asarray(steering, np.complex128)
    if a.ndim != 2:
        raise ValueError("doa: a steering table of shape %s ([n_dirs][n])" % (a.shape,))
    return np.ascontiguousarray(a.T)


def doa_scan_eval(vectors, g, steering, inverse=False):
    """rts_doa_scan_eval (pure host): q[dir] = sum_k g[k] |sum_rx conj(v_k[rx]) a_dir[rx]|^2 of the vectors complex [m][n], the weights
    g [m] and the host steering table complex [n_dirs][n] (steering()'s rows); 1 / q with inverse (q = 0 gives +inf): float64 [n_dirs]"""
    v = np.ascontiguousarray(np.asarray(vectors, np.complex128)); g = np.ascontiguousarray(np.asarray(g, np.float64).ravel())
    a = _steering_table(steering)
    if v.ndim != 2 or v.shape[1] != a.shape[0] or len(g) != v.shape[0]:
        raise ValueError("doa_scan_eval: vectors of shape %s, %d weights, a table of %d elements" % (v.shape, len(g), a.shape[0]))
    out = np.zeros(a.shape[1], np.float64)
    check(L.lib().rts_doa_scan_eval(ptr(v.view(np.float64)), ptr(g), v.shape[1], v.shape[0], ptr(a.view(np.float64)), a.shape[1],
                                    L.RTS_DOA_INVERSE if inverse else 0, ptr(out)))
    return out


_DOA_METHODS = {"bartlett": L.RTS_DOA_BARTLETT, "capon": L.RTS_DOA_CAPON, "music": L.RTS_DOA_MUSIC}


def doa_weights(method, values, n_sources=0, loading=0.0):
    """rts_doa_weights (pure host): a spectrum ("bartlett", "capon", "music") as the scan's (first vector, g [m], inverse) from the
    eigenvalues in eig_eval's order: Bartlett g = lambda over all vectors, Capon g = 1 / (lambda + loading) over all and inverse,
    MUSIC g = 1 over the vectors from n_sources on and inverse"""
    values = np.ascontiguousarray(np.asarray(values, np.float64).ravel())
    first, m, flags = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0); g = np.zeros(max(len(values), 1), np.float64)
    check(L.lib().rts_doa_weights(_DOA_METHODS.get(method, method), ptr(values), len(values), int(n_sources), float(loading),
                                  C.byref(first), C.byref(m), ptr(g), C.byref(flags)))
    return first.value, g[:m.value].copy(), bool(flags.value & L.RTS_DOA_INVERSE)


def source_count(values, K, criterion="mdl"):
    """rts_source_count (pure host): the number of sources by Wax and Kailath's "aic" or "mdl" from the eigenvalues in descending
    order (all > 0) and the number of snapshots K"""
    values = np.ascontiguousarray(np.asarray(values, np.float64).ravel())
    k = C.c_uint32(0)
    check(L.lib().rts_source_count(ptr(values), len(values), int(K), {"aic": L.RTS_DOA_AIC, "mdl": L.RTS_DOA_MDL}.get(criterion, criterion), C.byref(k)))
    return k.value


def _st_cov_params(taps, source, first, count, first_bin, n_bins, skip, device_in, n_rows_in):
    """RtsStCovParams: _cov_params' fields (the rows are the span the snapshots lie in) and the taps"""
    c = _cov_params(source, first, count, first_bin, n_bins, skip, device_in, n_rows_in)
    p = L.RtsStCovParams()
    for name in ("source", "n_rows_in", "first_row", "n_rows", "first_bin", "n_bins", "skip_first_bin", "skip_n_bins", "device_in"):
        setattr(p, name, getattr(c, name))
    p.n_taps = int(taps)
    return p


def st_covariance_eval(inp, taps, first=0, count=None, first_bin=0, n_bins=None, skip=None):
    """rts_st_covariance_eval (pure host): the sample covariance of the snapshots stacked over the receivers and `taps` consecutive
    rows, x[m n_rx + rx] = z[rx][p + m][b], of a host array [n_rx][n_rows][n_bins] (complex) -- start rows first .. first + count - taps
    of the span of count rows (default: to the last), bins as covariance_eval: complex [taps n_rx][taps n_rx]"""
    inp = np.ascontiguousarray(np.asarray(inp, np.complex128))
    n_rx, rows, nb = inp.shape
    q = L.RtsCubeParams(n_rx, rows, nb, 0, 0.0, 1.0)
    p = _st_cov_params(taps, "cube", first, count, first_bin, n_bins, skip, None, 0)
    D = n_rx * max(int(taps), 0)
    out = np.zeros((D, D), np.complex128)
    check(L.lib().rts_st_covariance_eval(C.byref(q), ptr(inp.view(np.float64)), rows, C.byref(p), ptr(out.view(np.float64))))
    return out


def _st_apply_params(weights, taps, n_rx, source, first, count, power, device_in, n_rows_in):
    """RtsStApplyParams and the weight array it points to (keep it alive for the call); count None: to the source's last row"""
    w = np.ascontiguousarray(np.asarray(weights, np.complex128))
    if w.ndim != 2 or w.shape[1] != int(taps) * n_rx:
        raise ValueError("st_apply: weights of shape %s for %d taps of %d receivers ([n_filters][taps n_rx])" % (w.shape, taps, n_rx))
    p = L.RtsStApplyParams()
    p.n_filters, p.source, p.n_taps = w.shape[0], _BEAM_SOURCES.get(source, source), int(taps)
    p.first_row, p.n_rows, p.n_rows_in = int(first), int(count or 0), int(n_rows_in)
    p.flags = L.RTS_BEAM_POWER if power else 0
    p.weights = ptr(w.view(np.float64))
    p.device_in = device_in if device_in else None
    return p, w


def st_apply_eval(inp, weights, taps, first=0, count=None, power=False):
    """rts_st_apply_eval (pure host): y[f][p] = sum_d conj(w[f][d]) x[d] over the stacked snapshots (st_covariance_eval) of rows
    first .. first + count - 1 (default: to the last) of a host array [n_rx][n_rows][n_bins] (complex), weights complex
    [n_filters][taps n_rx]: complex [n_filters][count - taps + 1][n_bins], or its power (float64, same shape) with power"""
    inp = np.ascontiguousarray(np.asarray(inp, np.complex128))
    n_rx, rows, nb = inp.shape
    q = L.RtsCubeParams(n_rx, rows, nb, 0, 0.0, 1.0)
    p, keep = _st_apply_params(weights, taps, n_rx, "cube", first, count, power, None, 0)
    out = _beam_out(p.n_filters, (p.n_rows if p.n_rows else rows - p.first_row) - p.n_taps + 1, nb, power, False)
    check(L.lib().rts_st_apply_eval(C.byref(q), ptr(inp.view(np.float64)), rows, C.byref(p), ptr(out.view(np.float64))))
    return out


def st_steering(spatial, dopplers, taps, tap_taper=None):
    """rts_st_steering_make (pure host): space-time steering rows temporal (x) spatial for spatial steering rows complex [n_beams][n_rx]
    (steering), Doppler frequencies [n_doppler] in cycles per pulse and an optional real taper over the taps: complex
    [n_beams n_doppler][taps n_rx], row beam n_doppler + k; y = sum conj(w) x peaks at a scatterer of that direction and frequency"""
    a = np.ascontiguousarray(np.atleast_2d(np.asarray(spatial, np.complex128)))
    f = np.ascontiguousarray(np.asarray(dopplers, np.float64).ravel())
    t = None if tap_taper is None else np.ascontiguousarray(np.asarray(tap_taper, np.float64).ravel())
    if t is not None and len(t) != int(taps):
        raise ValueError("st_steering: a taper of %d values for %d taps" % (len(t), taps))
    out = np.zeros((a.shape[0] * len(f), max(int(taps), 0) * a.shape[1]), np.complex128)
    check(L.lib().rts_st_steering_make(ptr(a.view(np.float64)), a.shape[1], a.shape[0], ptr(f), len(f), int(taps), ptr(t), ptr(out.view(np.float64))))
    return out


def device_count():
    n = C.c_int(0)
    rc = L.lib().rts_device_count(C.byref(n))
    return n.value if rc == 0 else 0


import os as _os
_PY_LAP = {} if _os.environ.get("RTS_PY_LAP") == "1" else None


# ------------------------------------------------------------------------------- the tracer handle
class Tracer:
    """One RtsHandle: scene + receivers + per-pulse launch on one GPU."""

    def __init__(self, width, max_refl, max_refr=0, smooth=True, device=0, keep_all=False, count_traversal=False, device_build=None, pre_filter=True, horizon=True, horizon_sectors=True):
        p = L.RtsParams(width, max_refl, max_refr, 1 if smooth else 0, device,
                        (L.RTS_FLAG_KEEP_ALL_RAYS if keep_all else 0) | (L.RTS_FLAG_COUNT_TRAVERSAL if count_traversal else 0) |
                        (0 if device_build is None else (L.RTS_FLAG_DEVICE_BUILD if device_build else L.RTS_FLAG_HOST_BUILD)) |      # None: the library's default (device)
                         (0 if pre_filter else L.RTS_FLAG_NO_PREFILTER) | (0 if horizon else L.RTS_FLAG_NO_HORIZON) | (0 if horizon_sectors else L.RTS_FLAG_NO_HORIZON_SECTORS))
        self.h = C.c_void_p()
        check(L.lib().rts_create(C.byref(p), C.byref(self.h)))
        self.width = width; self.max_refl = max_refl; self.depth = max_refl + (2 if max_refr else 0)
        self.n_targets = 0; self.keep_all = keep_all; self.device = device
        self._keep = []

    def close(self):
        if self.h:
            L.lib().rts_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, meshes):
        """meshes: list of dict(tris, verts, normals, refl_coeff, refr_index) in the target's own frame."""
        arr = (L.RtsMesh * max(len(meshes), 1))()
        keep = []
        for i, m in enumerate(meshes):
            t = np.ascontiguousarray(m["tris"], np.uint32); v = np.ascontiguousarray(m["verts"], np.float64)
            n = np.ascontiguousarray(m["normals"], np.float64)
            keep += [t, v, n]
            arr[i] = L.RtsMesh(t.ctypes.data, v.ctypes.data, n.ctypes.data, t.shape[0], v.shape[0], n.shape[0], 0,
                               float(m.get("refl_coeff", 1.0)), float(m.get("refr_index", 1.0)))
        check(L.lib().rts_set_scene(self.h, arr, len(meshes)))
        self.n_targets = len(meshes)

    def horizon(self, n_prims):
        """the scene's per-primitive isotropic horizon, [n_prims][2] = (S+, S-) by global primitive id: per side the largest of its
        four sectors (rts_get_horizon)"""
        out = np.zeros((int(n_prims), 2), np.float32)
        check(L.lib().rts_get_horizon(self.h, ptr(out), int(n_prims)))
        return out

    def horizon_sectors(self, n_prims):
        """the horizon by azimuth sector as the leaf records carry it, uint8 [n_prims][2][4] = side (+, -), quadrant of the in-plane
        azimuth in the primitive's frame (e0, n x e0); a byte b stands for b / 255 (rts_get_horizon_sectors)"""
        out = np.zeros((int(n_prims), 2, 4), np.uint8)
        check(L.lib().rts_get_horizon_sectors(self.h, ptr(out), int(n_prims)))
        return out

    def walk_stats(self):
        """the counting build's walk statistics of the last launch (rts_get_walk_stats), twelve values"""
        ls = (C.c_uint64 * 12)()
        check(L.lib().rts_get_walk_stats(self.h, ls, 12))
        return [int(v) for v in ls]

    def share_scene(self, other):
        """rts_share_scene: use `other`'s immutable scene (meshes, hierarchy, leaf order) instead of an own copy"""
        check(L.lib().rts_share_scene(self.h, other.h))
        self.n_targets = other.n_targets

    def scene_info(self):
        s = L.RtsSceneInfo()
        check(L.lib().rts_scene_info(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in L.RtsSceneInfo._fields_}

    def set_receivers(self, spheres):
        arr = (L.RtsReceiverSphere * max(len(spheres), 1))()
        for i, s in enumerate(spheres):
            arr[i] = L.RtsReceiverSphere((C.c_double * 3)(*s["centre"]), s["radius"], s["minTheta"], s["maxTheta"],
                                         s["minPhi"], s["maxPhi"])
        check(L.lib().rts_set_receivers(self.h, arr, len(spheres)))

    def trace(self, origin, tx_span, tx_dir, motion=None, ray_first=0, ray_count=0, want_stats=True, interleave=None):
        """motion: list of dict(position, velocity[, rotation(9)]) per target, or None to keep placement."""
        check(L.lib().rts_trace_pulse(self.h, C.byref(self._pulse(origin, tx_span, tx_dir, motion, ray_first, ray_count, interleave))))
        return self.stats() if want_stats else None     # reading the stage timers drains the stream

    def reserve(self, n_rays=0):
        """rts_reserve: allocate the per-launch device buffers now (0 = W^3 launch indices)"""
        check(L.lib().rts_reserve(self.h, n_rays))

    def trace_begin(self, origin, tx_span, tx_dir, motion=None, ray_first=0, ray_count=0, interleave=None):
        """enqueue a pulse (rts_trace_pulse_begin); trace_end() -- or any accessor -- completes it"""
        if _PY_LAP is None:
            check(L.lib().rts_trace_pulse_begin(self.h, C.byref(self._pulse(origin, tx_span, tx_dir, motion, ray_first, ray_count, interleave))))
            return
        import time                                                  # RTS_PY_LAP=1: where this call's time goes on the Python side
        t0 = time.perf_counter(); p = self._pulse(origin, tx_span, tx_dir, motion, ray_first, ray_count, interleave)
        t1 = time.perf_counter(); f = L.lib().rts_trace_pulse_begin
        t2 = time.perf_counter(); rc = f(self.h, C.byref(p))
        t3 = time.perf_counter(); check(rc)
        t4 = time.perf_counter()
        for k, v in zip(("marshal", "lookup", "call", "check"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            _PY_LAP[k] = _PY_LAP.get(k, 0.0) + v
        _PY_LAP["n"] = _PY_LAP.get("n", 0) + 1

    def block_timeline(self):
        """rts_get_block_timeline (a tracer created with RTS_TIMELINE_BLOCKS=1): dict of the last launch's block start / end times in us after the first start"""
        out = np.zeros(9, np.float64)
        check(L.lib().rts_get_block_timeline(self.h, ptr(out), 9))
        return dict(zip(("start_first", "start_p50", "start_last", "end_first", "end_p10", "end_p50", "end_p90", "end_last", "blocks"), out.tolist()))

    def trace_end(self):
        check(L.lib().rts_trace_pulse_end(self.h))

    # ---- ray sharding dealt by last-seen cost (rts_amd.h: rts_tile_records_get / _set, rts_set_tile_list; deal_tiles below)
    def tile_records_get(self):
        """cost records (uint32 per 64 launch indices) of the tiles this tracer's LAST launch traced, 0 elsewhere"""
        n = (self.width ** 3 + 63) // 64
        out = np.zeros(n, np.uint32)
        check(L.lib().rts_tile_records_get(self.h, ptr(out), n))
        return out

    def tile_records_set(self, records):
        r = np.ascontiguousarray(records, np.uint32)
        check(L.lib().rts_tile_records_set(self.h, ptr(r), r.shape[0]))

    def set_tile_list(self, tile, tile_ids):
        """the plan tiles (of `tile` launch indices, ascending) that launches with interleave=(tile, INTERLEAVE_LIST, 0) trace; no ids: an
        empty list (such launches trace nothing); tile = 0: no list any more"""
        ids = np.ascontiguousarray(tile_ids, np.uint32)
        check(L.lib().rts_set_tile_list(self.h, tile, ptr(ids) if ids.shape[0] else None, ids.shape[0]))

    def link(self, other):
        """rts_link_handles: trace kernels of linked tracers run one at a time, everything else overlaps"""
        check(L.lib().rts_link_handles(self.h, other.h))

    def _pulse(self, origin, tx_span, tx_dir, motion, ray_first, ray_count, interleave):
        # ONE RtsPulse and ONE motion array per tracer, refilled per call: the library copies what it needs before
        # rts_trace_pulse_begin returns, and a per-call ctypes allocation is a gc-tracked object -- in a long pulse loop the
        # collector's full passes over everything torch has imported then land in this function (0.15 ms per call at 256 pulses)
        p = self._pulse_struct = getattr(self, "_pulse_struct", None) or L.RtsPulse()
        p.ray_origin[:] = origin; p.tx_span[:] = tx_span; p.tx_dir[:] = tx_dir
        p.ray_first = ray_first; p.ray_count = ray_count
        p.interleave_tile, p.interleave_parts, p.interleave_part = interleave if interleave is not None else (0, 0, 0)      # (tile, parts, part)
        if motion is not None:
            assert len(motion) == self.n_targets
            marr = getattr(self, "_motion_arr", None)
            if marr is None or len(marr) != max(len(motion), 1):
                marr = self._motion_arr = (L.RtsTargetMotion * max(len(motion), 1))()
                self._motion_ptr = C.cast(marr, C.POINTER(L.RtsTargetMotion))
            for i, m in enumerate(motion):
                q = marr[i]
                q.position[:] = m["position"]; q.velocity[:] = m.get("velocity", (0.0, 0.0, 0.0))
                rot = m.get("rotation")
                if rot is not None:
                    q.rotation[:] = np.asarray(rot, np.float64).reshape(9).tolist(); q.has_rotation = 1
                else:
                    q.has_rotation = 0
            p.motion = self._motion_ptr
        else:
            p.motion = None
        return p

    def stats(self):
        s = L.RtsStats()
        check(L.lib().rts_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in L.RtsStats._fields_}

    def stats_raw(self):
        """rts_get_stats into ONE struct kept by the tracer (a caller in a per-pulse loop reads the few fields it wants)"""
        s = getattr(self, "_stats_struct", None)
        if s is None:
            s = self._stats_struct = L.RtsStats()
        check(L.lib().rts_get_stats(self.h, C.byref(s)))
        return s

    def received_count(self):
        n = C.c_uint64(0)
        check(L.lib().rts_received_count(self.h, C.byref(n)))
        return n.value

    def received(self):
        R = self.received_count(); D = self.depth
        rays = np.zeros(R, PRD_DTYPE); paths = np.zeros((R, D), np.int32); ang = np.zeros((R, D, 2)); slots = np.zeros(R, np.uint64)
        check(L.lib().rts_get_received(self.h, ptr(rays), ptr(paths), ptr(ang), ptr(slots), R))
        return dict(results=rays, path=paths, rcs_angle=ang, slots=slots)

    def received_prefetch(self):
        """rts_received_prefetch: the pulse in flight delivers its received set into the handle's pinned host mirror"""
        check(L.lib().rts_received_prefetch(self.h))

    def received_view(self):
        """rts_received_view: COPIES of the mirror's records (the views themselves only live until the next pulse)"""
        pr, pp, pa, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(); n = C.c_uint64(0)
        check(L.lib().rts_received_view(self.h, C.byref(pr), C.byref(pp), C.byref(pa), C.byref(ps), C.byref(n)))
        R = n.value; D = self.depth

        def arr(p, dtype, shape):
            count = int(np.prod(shape))
            if count == 0 or not p.value:
                return np.zeros(shape, dtype)
            return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(p.value), dtype=dtype).reshape(shape).copy()
        return dict(results=arr(pr, PRD_DTYPE, (R,)), path=arr(pp, np.int32, (R, D)), rcs_angle=arr(pa, np.float64, (R, D, 2)), slots=arr(ps, np.uint64, (R,)))

    def finalise_values(self, power, doppler):
        p = np.ascontiguousarray(power, np.float64); d = np.ascontiguousarray(doppler, np.float64)
        check(L.lib().rts_finalise_values(self.h, ptr(p), ptr(d), len(p)))

    def aggregated_view(self):
        ps = [C.c_void_p() for _ in range(5)]; n = C.c_uint64(0)
        check(L.lib().rts_aggregated_view(self.h, *[C.byref(q) for q in ps], C.byref(n)))
        R = n.value
        out = {}
        for name, q, dt in zip(("power", "doppler", "delay", "phase", "pathMatch"), ps, (np.float64,) * 4 + (np.int32,)):
            out[name] = np.frombuffer((C.c_char * (R * np.dtype(dt).itemsize)).from_address(q.value), dtype=dt).copy() if R and q.value else np.zeros(R, dt)
        return out

    def all_rays(self, n_rays, rows=None):
        """full per-row buffers (keep_all): rows * n_rays records (rows = max_refl + 3 with refraction, else 1)"""
        D = self.depth; H = self.max_refl + 1
        rows = rows if rows is not None else (self.max_refl + 3 if self.depth > self.max_refl else 1)
        n = n_rays * rows
        res = np.zeros(n, PRD_DTYPE); path = np.zeros((n, D), np.int32); ang = np.zeros((n, D, 2))
        hp = np.zeros((n_rays, H), np.int32); ht = np.zeros((n_rays, H), np.float32)
        check(L.lib().rts_get_all_rays(self.h, ptr(res), ptr(path), ptr(ang), ptr(hp), ptr(ht), n))
        return dict(results=res, path=path, rcs_angle=ang, hit_prim=hp, hit_t=ht)

    def finalise_uniform(self, rcs_per_target, wavelength, gt, gr, carrier, cspeed):
        r = np.ascontiguousarray(rcs_per_target, np.float64) if rcs_per_target is not None else None
        check(L.lib().rts_finalise_uniform(self.h, ptr(r), wavelength, gt, gr, carrier, cspeed))

    def trace_end_uniform(self, rcs_per_target, wavelength, gt, gr, carrier, cspeed, cube_pulse=-1, recv_index_base=0):
        """rts_trace_pulse_end + rts_finalise_uniform (+ rts_cube_accumulate) + rts_aggregate in one call that does not wait for the
        trace when the handle's previous pulse received few rays; received_count() / stats() / groups() wait"""
        r = np.ascontiguousarray(rcs_per_target, np.float64) if rcs_per_target is not None else None
        check(L.lib().rts_trace_pulse_end_uniform(self.h, ptr(r), wavelength, gt, gr, carrier, cspeed, cube_pulse, recv_index_base))

    def set_patterns(self, tx, rx_list, rcs_list):
        """rts_set_patterns: the transmitter's, one per receiver and one per target (Pattern or RtsPattern)"""
        rx = (L.RtsPattern * max(len(rx_list), 1))(*[_pattern_desc(p) for p in rx_list])
        rcs = (L.RtsPattern * max(len(rcs_list), 1))(*[_pattern_desc(p) for p in rcs_list])
        check(L.lib().rts_set_patterns(self.h, C.byref(_pattern_desc(tx)), rx, len(rx_list), rcs, len(rcs_list)))

    @staticmethod
    def _pattern_pulse(rx_positions, rx_rotations, wavelength, carrier, cspeed):
        pos = np.ascontiguousarray(np.asarray(rx_positions, np.float64).reshape(-1, 3))
        rot = np.ascontiguousarray(np.asarray(rx_rotations, np.float64).reshape(-1, 4))
        return L.RtsPatternPulse(wavelength, carrier, cspeed, ptr(pos), ptr(rot)), (pos, rot)

    def finalise_patterns(self, rx_positions, rx_rotations, wavelength, carrier, cspeed):
        """rts_finalise_patterns: rx_positions [n_rx][3], rx_rotations [n_rx][4] = az, el at the pulse time, az_rate, el_rate (rad/s)"""
        q, keep = self._pattern_pulse(rx_positions, rx_rotations, wavelength, carrier, cspeed)
        check(L.lib().rts_finalise_patterns(self.h, C.byref(q)))

    def trace_end_patterns(self, rx_positions, rx_rotations, wavelength, carrier, cspeed, cube_pulse=-1, recv_index_base=0):
        """trace_end_uniform with the pattern finalisation"""
        q, keep = self._pattern_pulse(rx_positions, rx_rotations, wavelength, carrier, cspeed)
        check(L.lib().rts_trace_pulse_end_patterns(self.h, C.byref(q), cube_pulse, recv_index_base))

    def aggregate(self, cspeed, carrier, recv_index_base=0, fetch=True):
        """fetch=False: only enqueue (the library reads the group table when it is first asked for: groups())"""
        check(L.lib().rts_aggregate(self.h, cspeed, carrier, recv_index_base))
        return self.groups() if fetch else None

    def groups(self):
        n = C.c_uint32(0)
        check(L.lib().rts_group_count(self.h, C.byref(n)))
        g = np.zeros(max(n.value, 1), GROUP_DTYPE)
        check(L.lib().rts_get_groups(self.h, ptr(g), len(g)))
        return g[:n.value].copy()

    def aggregated(self):
        R = self.received_count()
        rays = np.zeros(R, PRD_DTYPE); delay = np.zeros(R); phase = np.zeros(R); pm = np.zeros(R, np.int32)
        check(L.lib().rts_get_aggregated(self.h, ptr(rays), ptr(delay), ptr(phase), ptr(pm), R))
        return dict(results=rays, delay=delay, phase=phase, pathMatch=pm)

    def cube_attach(self, n_rx, n_pulses, n_bins, t0, dt, device_ptr=None):
        """complex return cube [n_rx][n_pulses][n_bins]; device_ptr = data_ptr() of a zeroed complex128 device tensor, or None"""
        q = L.RtsCubeParams(n_rx, n_pulses, n_bins, 0, t0, dt)
        check(L.lib().rts_cube_attach(self.h, C.byref(q), C.c_void_p(device_ptr) if device_ptr else None))
        self._cube_shape = (n_rx, n_pulses, n_bins)

    def cube_accumulate(self, pulse_index, cspeed, carrier):
        check(L.lib().rts_cube_accumulate(self.h, pulse_index, cspeed, carrier))

    def cube_accumulate_paths(self, pulse_index):
        """one contribution per unique (receiver, path) of the pulse: the group values of rts_aggregate"""
        check(L.lib().rts_cube_accumulate_paths(self.h, pulse_index))

    def cube_doppler(self, n_fft, device_ptr=None, fetch=True):
        """slow-time DFT over the pulse axis (n_fft: power of two >= n_pulses): complex [n_rx][n_fft][n_bins]"""
        check(L.lib().rts_cube_doppler(self.h, n_fft, C.c_void_p(device_ptr) if device_ptr else None))
        self._doppler_n = n_fft
        if not fetch:
            return None
        out = np.zeros((self._cube_shape[0], n_fft, self._cube_shape[2], 2), np.float64)
        check(L.lib().rts_cube_doppler_get(self.h, ptr(out), out.size))
        return out[..., 0] + 1j * out[..., 1]

    def cube_set_waveform(self, w):
        """rts_cube_set_waveform: the waveform (Waveform or RtsWaveform) cube_render and cube_compress use"""
        check(L.lib().rts_cube_set_waveform(self.h, C.byref(_waveform_desc(w))))

    def cube_render(self, pulse, source="rays", cspeed=None, carrier=None, doppler=True):
        """rts_cube_render: the last pulse's contributions rendered with the waveform into row `pulse` of every receiver;
        source "rays" (every received ray: needs cspeed and carrier) or "paths" (one per group of rts_aggregate)"""
        src = {"rays": L.RTS_RENDER_RAYS, "paths": L.RTS_RENDER_PATHS}.get(source, source)
        if src == L.RTS_RENDER_RAYS and (cspeed is None or carrier is None):
            raise ValueError("cube_render(source='rays') needs cspeed and carrier")
        check(L.lib().rts_cube_render(self.h, pulse, src, L.RTS_RENDER_DOPPLER if doppler else 0,
                                      0.0 if cspeed is None else cspeed, 0.0 if carrier is None else carrier))

    def cube_render_beat(self, pulse, slope, duration, source="rays", cspeed=None, carrier=None, doppler=True):
        """rts_cube_render_beat: the last pulse's contributions as the dechirped beat signal of a chirp of `slope` Hz/s running for
        `duration` s, added into row `pulse` of every receiver; source "rays" (needs cspeed and carrier) or "paths" (one per group of
        rts_aggregate).  No waveform is needed."""
        p = _beat_params(slope, duration, source, doppler)
        if p.source == L.RTS_RENDER_RAYS and (cspeed is None or carrier is None):
            raise ValueError("cube_render_beat(source='rays') needs cspeed and carrier")
        check(L.lib().rts_cube_render_beat(self.h, pulse, C.byref(p), 0.0 if cspeed is None else cspeed, 0.0 if carrier is None else carrier))

    def cube_range_transform(self, n_fft, window=None, first=0, count=None, first_bin=0, n_samples=0, n_out=0, reverse=False, device_ptr=None,
                             fetch=True):
        """rts_cube_range_transform: the n_fft-point transform along the range axis of the attached cube's rows first .. first + count - 1
        (default: to the last), of the samples first_bin .. first_bin + n_samples - 1 (n_samples 0: to the row's end) tapered by window
        (an array of that many values, or None) and zero-padded; n_out bins kept (0: all), index-reversed with reverse (an up-chirp:
        beat_axis).  Into a caller complex128 device tensor [n_rx][count][n_out] (device_ptr; nothing is fetched) or the library's
        output, returned when fetch"""
        n_rx, n_p, nb = self._cube_shape
        p, keep = _range_params(n_fft, window, first, count, first_bin, n_samples, n_out, reverse, n_p, nb)
        check(L.lib().rts_cube_range_transform(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._range_shape = (n_rx, p.n_pulses, p.n_out if p.n_out else p.n_fft)
        return self.range_map() if fetch else None

    def range_map(self):
        """rts_cube_range_get: the library-owned output of the last cube_range_transform, complex [n_rx][count][n_out]"""
        out = np.zeros(getattr(self, "_range_shape", None) or (1, 1, 1), np.complex128)
        check(L.lib().rts_cube_range_get(self.h, ptr(out.view(np.float64)), 2 * out.size))
        return out

    def cube_beamform(self, weights, source="cube", first=0, count=None, power=False, peak=False, device_in=None, n_rows_in=0, device_ptr=None,
                      fetch=True):
        """rts_cube_beamform: beams y[b] = sum_rx conj(w[b][rx]) z[rx] over the receivers, weights complex [n_beams][n_rx] (steering), of
        rows first .. first + count - 1 (default: to the last) of the source: "cube" (the attached cube), "map" (the library-owned
        map of the last cube_doppler) or "pointer" (device_in = data_ptr() of a complex128 device tensor [n_rx][n_rows_in][n_bins]).
        Complex [n_beams][count][n_bins] -- the layout of a cube of n_beams receivers --, its power with power, or float64
        [count][n_bins][2] = (largest beam power, refined beam coordinate: beam_angles) with peak.  Into a caller device tensor
        (device_ptr; nothing is fetched) or the library's output, returned when fetch"""
        n_rx, n_p, nb = self._cube_shape
        p, keep = _beam_params(weights, n_rx, source, first, count, power, peak, device_in, n_rows_in)
        check(L.lib().rts_cube_beamform(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        rows = {L.RTS_BEAM_FROM_CUBE: n_p, L.RTS_BEAM_FROM_MAP: getattr(self, "_doppler_n", 0)}.get(p.source, p.n_rows_in)
        self._beam_shape = (p.n_beams, p.n_rows if p.n_rows else rows - p.first_row, nb, bool(power), bool(peak))
        return self.beam_map() if fetch else None

    def beam_map(self):
        """rts_cube_beam_get: the library-owned output of the last cube_beamform, in its form"""
        out = _beam_out(*(getattr(self, "_beam_shape", None) or (1, 1, 1, False, False)))
        check(L.lib().rts_cube_beam_get(self.h, ptr(out.view(np.float64)), out.view(np.float64).size))
        return out

    def cube_covariance(self, source="cube", first=0, count=None, first_bin=0, n_bins=None, skip=None, device_in=None, n_rows_in=0,
                        device_ptr=None, fetch=True):
        """rts_cube_covariance: the sample covariance of the receivers over the training cells -- rows first .. first + count - 1 and bins
        first_bin .. first_bin + n_bins - 1 (defaults: to the last) of the source ("cube", "map" or "pointer", as cube_beamform)
        without the bins skip = (first skipped bin, how many): the cells under test and their guard.  Complex [n_rx][n_rx] into a
        caller device tensor (device_ptr; nothing is fetched) or the library's output, returned when fetch"""
        p = _cov_params(source, first, count, first_bin, n_bins, skip, device_in, n_rows_in)
        check(L.lib().rts_cube_covariance(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._cov_n = self._cube_shape[0]
        return self.covariance() if fetch else None

    def covariance(self):
        """rts_cube_covariance_get: the library-owned output of the last cube_covariance, complex [n_rx][n_rx]"""
        n = getattr(self, "_cov_n", None) or 1
        out = np.zeros((n, n), np.complex128)
        check(L.lib().rts_cube_covariance_get(self.h, ptr(out.view(np.float64)), 2 * out.size))
        return out

    def cube_mvdr(self, steering, loading=0.0, device_cov=None, device_ptr=None, fetch=True):
        """rts_cube_mvdr: the MVDR weights of steering rows complex [n_beams][n_rx] (steering) from the library-owned covariance of the
        last cube_covariance, or from device_cov = data_ptr() of a complex128 device tensor [n_rx][n_rx]; loading is added to the
        covariance's diagonal (the cube's power units, e.g. cube_add_noise's noise_power).  Complex [n_beams][n_rx] into a caller
        device tensor (device_ptr; nothing is fetched) or the library's output, returned when fetch; a failed solve raises there"""
        p, keep = _mvdr_params(steering, 0 if device_cov else getattr(self, "_cov_n", 0), loading, device_cov)
        check(L.lib().rts_cube_mvdr(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._mvdr_shape = (p.n_beams, p.n_rx)
        return self.mvdr_weights() if fetch else None

    def mvdr_weights(self):
        """rts_cube_mvdr_get: the library-owned output of the last cube_mvdr, complex [n_beams][n_rx]: cube_beamform's weights"""
        out = np.zeros(getattr(self, "_mvdr_shape", None) or (1, 1), np.complex128)
        check(L.lib().rts_cube_mvdr_get(self.h, ptr(out.view(np.float64)), 2 * out.size))
        return out

    def cube_adaptive_beamform(self, steering, train=None, loading=0.0, **beamform_kwargs):
        """cube_covariance(**train) -> cube_mvdr(steering, loading) -> cube_beamform(the weights, **beamform_kwargs): beams whose
        weights are computed from the training cells `train` names (cube_covariance's keywords; default: every cell of the cube).
        The cube stays on the device; the weights (at most 64 KiB) pass through the host.  Returns cube_beamform's result."""
        self.cube_covariance(fetch=False, **(train or {}))
        w = self.cube_mvdr(steering, loading)
        return self.cube_beamform(w, **beamform_kwargs)

    def cube_eig(self, n=None, device_cov=None, device_values=None, device_vectors=None, fetch=True):
        """rts_cube_eig: the eigenpairs of the library-owned covariance of the last cube_covariance / cube_st_covariance, or of
        device_cov = data_ptr() of a complex128 device tensor [n][n] (n is needed then).  Into caller device tensors float64 [n] and
        complex128 [n][n] (device_values and device_vectors, both; nothing is fetched) or the library's outputs, returned when fetch:
        (eigenvalues descending, eigenvectors, ROW k the eigenvector of value k); a failed solve raises there"""
        if device_cov and not n:
            raise ValueError("cube_eig(device_cov=...) needs n")
        p = L.RtsEigParams()
        p.n, p.device_cov = int(n or 0), device_cov if device_cov else None
        check(L.lib().rts_cube_eig(self.h, C.byref(p), C.c_void_p(device_values) if device_values else None, C.c_void_p(device_vectors) if device_vectors else None))
        if device_values or device_vectors:
            return None
        self._eig_n = int(n) if device_cov else (getattr(self, "_cov_n", 0) or int(n or 0))
        return self.eigenpairs() if fetch else None

    def eigenpairs(self):
        """rts_cube_eig_get: the library-owned outputs of the last cube_eig: (eigenvalues float64 [n], eigenvectors complex [n][n])"""
        n = getattr(self, "_eig_n", None) or 1
        values = np.zeros(n, np.float64); vectors = np.zeros((n, n), np.complex128)
        check(L.lib().rts_cube_eig_get(self.h, ptr(values), ptr(vectors.view(np.float64)), n, 2 * n * n))
        return values, vectors

    def cube_doa_scan(self, steering, g, first_vector=0, inverse=False, n_dirs=None, device_vectors=None, n=None, device_ptr=None, fetch=True):
        """rts_cube_doa_scan: the angular spectrum q[dir] = sum_k g[k] |v_k^H a_dir|^2 (1 / q with inverse) through the rows first_vector ..
        first_vector + len(g) - 1 of the library-owned eigenvectors of the last cube_eig, or of device_vectors = data_ptr() of a
        complex128 device tensor [n][n] (n is needed then).  steering: a host table complex [n_dirs][n] (steering()'s rows), which is
        transposed and uploaded through torch, or data_ptr() of a complex128 device tensor in the scan's own element-major layout
        [n][n_dirs] (n_dirs is needed then).  Float64 [n_dirs] into a caller device tensor (device_ptr; nothing is fetched) or the
        library's output, returned when fetch"""
        g = np.ascontiguousarray(np.asarray(g, np.float64).ravel())
        if isinstance(steering, int):
            if not n_dirs:
                raise ValueError("cube_doa_scan(steering=<device pointer>) needs n_dirs")
            table = steering
        else:
            import torch
            a = _steering_table(steering)
            # the table lives on the handle until the next upload replaces it; torch's stream is not the handle's: the device-wide wait puts
            # the table in place before the scan reads it and ends the previous scan before its table goes
            self._doa_table = torch.from_numpy(a).to("cuda:%d" % self.device)
            torch.cuda.synchronize(self.device)
            table, n_dirs = self._doa_table.data_ptr(), a.shape[1]
        if device_vectors and not n:
            raise ValueError("cube_doa_scan(device_vectors=...) needs n")
        p = L.RtsDoaScanParams()
        p.n, p.first_vector, p.m, p.flags, p.n_dirs = int(n or 0), int(first_vector), len(g), L.RTS_DOA_INVERSE if inverse else 0, int(n_dirs)
        p.g, p.device_steering, p.device_vectors = ptr(g), table, device_vectors if device_vectors else None
        check(L.lib().rts_cube_doa_scan(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._doa_n = int(n_dirs)
        return self.doa_spectrum() if fetch else None

    def doa_spectrum(self):
        """rts_cube_doa_get: the library-owned output of the last cube_doa_scan, float64 [n_dirs]"""
        out = np.zeros(getattr(self, "_doa_n", None) or 1, np.float64)
        check(L.lib().rts_cube_doa_get(self.h, ptr(out), out.size))
        return out

    def cube_doa(self, steering, method="music", n_sources=None, loading=0.0, train=None):
        """cube_covariance(**train) -> cube_eig -> doa_weights(method, the eigenvalues, n_sources, loading) -> cube_doa_scan(steering):
        the angular spectrum ("music", "capon" or "bartlett") of the training cells `train` names (cube_covariance's keywords;
        default: every cell of the cube) over the host table steering [n_dirs][n_rx] (steering()'s rows).  n_sources None:
        source_count's MDL estimate from the eigenvalues and the number of training cells.  The cube stays on the device; the
        eigenvalues (at most 64) pass through the host.  Returns the spectrum float64 [n_dirs]."""
        train = dict(train or {})
        self.cube_covariance(fetch=False, **train)
        values, _ = self.cube_eig()
        if n_sources is None and method in ("music", L.RTS_DOA_MUSIC):
            n_rx, n_p, nb = self._cube_shape
            rows = {"cube": n_p, "map": getattr(self, "_doppler_n", 0)}.get(train.get("source", "cube"), train.get("n_rows_in", 0))
            K = (train.get("count") or rows - train.get("first", 0)) * ((train.get("n_bins") or nb - train.get("first_bin", 0)) - (train["skip"][1] if train.get("skip") else 0))
            n_sources = source_count(values, K, "mdl")
        first, g, inverse = doa_weights(method, values, n_sources or 0, loading)
        return self.cube_doa_scan(steering, g, first_vector=first, inverse=inverse)

    def cube_st_covariance(self, taps, source="cube", first=0, count=None, first_bin=0, n_bins=None, skip=None, device_in=None, n_rows_in=0,
                           device_ptr=None, fetch=True):
        """rts_cube_st_covariance: the sample covariance of the snapshots stacked over the receivers and `taps` consecutive rows of the
        source (st_covariance_eval; sources and training cells as cube_covariance, the rows being the span the snapshots lie in).
        Complex [taps n_rx][taps n_rx] into a caller device tensor (device_ptr; nothing is fetched) or the library's output, which
        is then the handle's covariance: covariance() returns it and cube_mvdr solves it"""
        p = _st_cov_params(taps, source, first, count, first_bin, n_bins, skip, device_in, n_rows_in)
        check(L.lib().rts_cube_st_covariance(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._cov_n = self._cube_shape[0] * p.n_taps
        return self.covariance() if fetch else None

    def cube_st_apply(self, weights, taps, source="cube", first=0, count=None, power=False, device_in=None, n_rows_in=0, device_ptr=None, fetch=True):
        """rts_cube_st_apply: the space-time filters y[f][p] = sum_d conj(w[f][d]) x[d], weights complex [n_filters][taps n_rx], over
        the stacked snapshots of rows first .. first + count - 1 (default: to the last) of the source (as cube_beamform).  Complex
        [n_filters][count - taps + 1][n_bins] -- the layout of a cube of n_filters receivers and count - taps + 1 pulses --, or its
        power with power.  Into a caller device tensor (device_ptr; nothing is fetched) or the library's output, returned when fetch"""
        n_rx, n_p, nb = self._cube_shape
        p, keep = _st_apply_params(weights, taps, n_rx, source, first, count, power, device_in, n_rows_in)
        check(L.lib().rts_cube_st_apply(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        rows = {L.RTS_BEAM_FROM_CUBE: n_p, L.RTS_BEAM_FROM_MAP: getattr(self, "_doppler_n", 0)}.get(p.source, p.n_rows_in)
        self._st_shape = (p.n_filters, (p.n_rows if p.n_rows else rows - p.first_row) - p.n_taps + 1, nb, bool(power), False)
        return self.st_map() if fetch else None

    def st_map(self):
        """rts_cube_st_get: the library-owned output of the last cube_st_apply, in its form"""
        out = _beam_out(*(getattr(self, "_st_shape", None) or (1, 1, 1, False, False)))
        check(L.lib().rts_cube_st_get(self.h, ptr(out.view(np.float64)), out.view(np.float64).size))
        return out

    def cube_stap(self, spatial_steering, dopplers, taps, train=None, loading=0.0, **apply_kwargs):
        """cube_st_covariance(taps, **train) -> cube_mvdr(st_steering(spatial_steering, dopplers, taps), loading) on the library-owned
        covariance -> cube_st_apply(the weights, taps, **apply_kwargs): space-time filters, one per (beam, Doppler) pair in
        st_steering's order, whose weights are computed from the training snapshots `train` names (cube_st_covariance's keywords;
        default: every snapshot of the cube).  The cube stays on the device; the weights (at most 64 KiB) pass through the host.
        Returns cube_st_apply's result."""
        self.cube_st_covariance(taps, fetch=False, **(train or {}))
        w = self.cube_mvdr(st_steering(spatial_steering, dopplers, taps), loading)
        return self.cube_st_apply(w, taps, **apply_kwargs)

    def cube_compress(self, first=0, count=None):
        """rts_cube_compress: matched filter of rows first .. first + count - 1 (default: to the last pulse), in place"""
        if count is None:
            count = self._cube_shape[1] - first
        check(L.lib().rts_cube_compress(self.h, first, count))

    def cube_bank(self, waves, code=None, first=0, count=None, device_ptr=None, fetch=True):
        """rts_cube_bank: the matched-filter bank -- every row of rows first .. first + count - 1 (default: to the last pulse) of every
        receiver of the attached cube correlated with each of the waveforms (one per transmitter that was rendered into the cube),
        then multiplied by conj(code[t][p]) (code complex [n_waves][count], None: no multiply): complex [n_waves * n_rx][count][n_bins],
        virtual element t * n_rx + r, into a caller complex128 device tensor (device_ptr; nothing is fetched) or the library's output,
        returned when fetch.  The cube is not changed.  Attached as a cube of n_waves * n_rx receivers (a caller-owned output: the
        attach ends the library's), the array methods run on the virtual array (virtual_positions)"""
        p, keep = _bank_params(waves, code, first, count, self._cube_shape[1])
        check(L.lib().rts_cube_bank(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._bank_shape = (p.n_waves * self._cube_shape[0], p.n_pulses, self._cube_shape[2])
        return self.bank_map() if fetch else None

    def bank_map(self):
        """rts_cube_bank_get: the library-owned output of the last cube_bank, complex [n_waves * n_rx][count][n_bins]"""
        out = np.zeros(getattr(self, "_bank_shape", None) or (1, 1, 1), np.complex128)
        check(L.lib().rts_cube_bank_get(self.h, ptr(out.view(np.float64)), 2 * out.size))
        return out

    def cube_cancel(self, ref_rx, n_taps, rows_per_block=0, first=0, count=None, rx=None, loading=0.0):
        """rts_cube_cancel: batch ECA in place on the attached cube -- per block of rows_per_block rows (0: the whole span) of rows
        first .. first + count - 1 (default: to the last pulse) the least-squares fit of the n_taps lagged copies of receiver
        ref_rx's row is subtracted from the receivers rx (None: all but ref_rx; indices or a mask).  The block length is the Doppler
        notch: about one cycle per block around 0, over the lags below n_taps"""
        p = _cancel_params(ref_rx, n_taps, first, count, rows_per_block, rx, loading, self._cube_shape[1])
        check(L.lib().rts_cube_cancel(self.h, C.byref(p)))
        self._cancel_shape = (self._cube_shape[0], _cancel_blocks(p.n_pulses, p.rows_per_block), p.n_taps)

    def cancel_info(self):
        """rts_cube_cancel_info: (n_blocks, n_failed) of the last cube_cancel; a failed block (a pivot of the factor not finite or
        not > 0) was left unchanged and its coefficients are 0"""
        nblk, nfail = C.c_uint32(0), C.c_uint32(0)
        check(L.lib().rts_cube_cancel_info(self.h, C.byref(nblk), C.byref(nfail)))
        return nblk.value, nfail.value

    def cancel_coeffs(self):
        """rts_cube_cancel_coeffs_get: the coefficients of the last cube_cancel, complex [n_rx][n_blocks][n_taps] (zeros for the
        reference and for receivers that were not cancelled)"""
        out = np.zeros(getattr(self, "_cancel_shape", None) or (1, 1, 1), np.complex128)
        check(L.lib().rts_cube_cancel_coeffs_get(self.h, ptr(out.view(np.float64)), 2 * out.size))
        return out

    def cube_xcorr(self, ref_rx, n_lags, first_lag=0, first=0, count=None, device_ptr=None, fetch=True):
        """rts_cube_xcorr: every row of rows first .. first + count - 1 (default: to the last pulse) of every receiver correlated with
        receiver ref_rx's row of the same pulse at the lags first_lag .. first_lag + n_lags - 1: complex [n_rx][count][n_lags], into
        a caller complex128 device tensor (device_ptr; nothing is fetched) or the library's output, returned when fetch.  Attached
        as a cube of n_bins = n_lags, t0 = first_lag * dt, cube_doppler makes the range-Doppler map of it"""
        p = _xcorr_params(ref_rx, n_lags, first_lag, first, count, self._cube_shape[1])
        check(L.lib().rts_cube_xcorr(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._xcorr_shape = (self._cube_shape[0], p.n_pulses, p.n_lags)
        return self.xcorr_map() if fetch else None

    def xcorr_map(self):
        """rts_cube_xcorr_get: the library-owned output of the last cube_xcorr, complex [n_rx][count][n_lags]"""
        out = np.zeros(getattr(self, "_xcorr_shape", None) or (1, 1, 1), np.complex128)
        check(L.lib().rts_cube_xcorr_get(self.h, ptr(out.view(np.float64)), 2 * out.size))
        return out

    def cube_passive(self, ref_rx, n_taps, n_lags, rows_per_block=0, first_lag=0, first=0, count=None, rx=None, loading=0.0, device_ptr=None,
                     fetch=True):
        """cube_cancel(ref_rx, n_taps, rows_per_block, first, count, rx, loading) -> cube_xcorr(ref_rx, n_lags, first_lag, first,
        count, device_ptr, fetch): the passive radar's two steps on the attached cube; returns cube_xcorr's result"""
        self.cube_cancel(ref_rx, n_taps, rows_per_block, first, count, rx, loading)
        return self.cube_xcorr(ref_rx, n_lags, first_lag, first, count, device_ptr, fetch)

    def cube_add_noise(self, noise_power, seed, first=0, count=None):
        """rts_cube_add_noise: complex Gaussian noise of power noise_power (E|n|^2) added to rows first .. first + count - 1 (default:
        to the last pulse) of every receiver; each sample a function of (seed, flat cube index) alone"""
        if count is None:
            count = self._cube_shape[1] - first
        check(L.lib().rts_cube_add_noise(self.h, first, count, float(noise_power), int(seed)))

    def cube_add_sources(self, spatial, power, doppler, rho=None, range_profile=None, seed=0):
        """rts_cube_add_sources: K independent first-order Gaussian patches (clutter, jammers) added to every row of the attached cube
        on the device; the arguments are sources_eval's.  Each draw is a function of (seed, bin, pulse, patch) alone and the sum over
        the patches runs in one fixed order, so the result does not depend on the launch"""
        shape = getattr(self, "_cube_shape", None)
        if shape is None:
            check(L.lib().rts_cube_add_sources(self.h, None))          # (the library's own refusal: no cube)
        p, keep = _source_params(spatial, power, doppler, rho, range_profile, seed, shape[0], shape[2])
        check(L.lib().rts_cube_add_sources(self.h, C.byref(p)))

    def cube_detect(self, guard=(2, 2), train=(8, 4), mode="ca", pfa=None, alpha=None, local_max=True, pri=0.0, device_ptr=None,
                    n_doppler=None, max_detections=0, fetch=True):
        """rts_cube_detect + rts_cube_detections_get: CFAR on the handle's last cube_doppler map (device_ptr None) or on a caller
        complex128 device map [n_rx][n_doppler][n_bins]; guard and train are (range, Doppler) cells on each side; mode "ca", "go"
        or "so"; exactly one of pfa (CA) and alpha.  Returns a DETECTION_DTYPE array in flat (rx, doppler_bin, range_bin) order."""
        p = _cfar_params(L.RtsCfarParams(), guard, train, pfa, alpha, local_max, pri, max_detections)
        p.mode = {"ca": L.RTS_CFAR_CA, "go": L.RTS_CFAR_GO, "so": L.RTS_CFAR_SO}.get(mode, mode)
        return self._detect(L.lib().rts_cube_detect, "cube_detect", p, device_ptr, n_doppler, fetch)

    def cube_detect_os(self, guard=(2, 2), train=(8, 4), rank=None, pfa=None, alpha=None, local_max=True, pri=0.0, device_ptr=None,
                       n_doppler=None, max_detections=0, fetch=True):
        """rts_cube_detect_os + rts_cube_detections_get: ordered-statistic CFAR on the handle's last cube_doppler map (device_ptr None)
        or on a caller complex128 device map [n_rx][n_doppler][n_bins]; guard and train are (range, Doppler) cells on each side; rank
        is the rank in a full window of N0 training cells (None: (3 N0) // 4); exactly one of pfa and alpha.  Returns a
        DETECTION_DTYPE array in flat (rx, doppler_bin, range_bin) order."""
        p = _cfar_os_params(guard, train, rank, pfa, alpha, local_max, pri, max_detections)
        return self._detect(L.lib().rts_cube_detect_os, "cube_detect_os", p, device_ptr, n_doppler, fetch)

    def _detect(self, call, who, p, device_ptr, n_doppler, fetch):
        """either detector on the handle's map (device_ptr None) or the caller's, which needs n_doppler; the list when fetch"""
        if device_ptr and n_doppler is None:
            raise ValueError("%s(device_ptr=...) needs n_doppler" % who)
        check(call(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None, int(n_doppler or 0)))
        return self.detections() if fetch else None

    def detections(self):
        """rts_cube_detections_get: the list of the last cube_detect or cube_detect_os (every stored record; raises when max_detections cut it)"""
        n = C.c_uint32(0)
        rc = L.lib().rts_cube_detections_get(self.h, None, 0, C.byref(n))
        if rc not in (L.RTS_OK, L.RTS_ERR_CAPACITY):
            check(rc)
        out = np.zeros(max(n.value, 1), L.DETECTION_DTYPE)
        check(L.lib().rts_cube_detections_get(self.h, ptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def cube_plots(self, link=(1, 1), min_cells=1, pri=0.0, max_plots=0, device_list=None, n_list=0, n_doppler=0, fetch=True):
        """rts_cube_plots + rts_cube_plots_get: the connected components of the handle's detection list (device_list None) or of a
        caller-owned device array of n_list RtsDetection records on a map of n_doppler rows, one record per component; link is the
        adjacency's reach (range, Doppler) in cells.  Detect without local_max first.  Returns a PLOT_DTYPE array in ascending
        first_index."""
        p = _plot_params(link, min_cells, pri, max_plots, device_list, n_list, n_doppler)
        check(L.lib().rts_cube_plots(self.h, C.byref(p)))
        return self.plots() if fetch else None

    def plots(self):
        """rts_cube_plots_get: the plots of the last cube_plots (every stored record; raises when max_plots cut them or the detection
        list they were made from was truncated)"""
        n = C.c_uint32(0)
        rc = L.lib().rts_cube_plots_get(self.h, None, 0, C.byref(n))
        if rc not in (L.RTS_OK, L.RTS_ERR_CAPACITY):
            check(rc)
        out = np.zeros(max(n.value, 1), L.PLOT_DTYPE)
        check(L.lib().rts_cube_plots_get(self.h, ptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def cube_track(self, time, sigma, gate=9.21, q=0.0, delay_rate_per_hz=0.0, doppler_period=0.0, confirm_hits=3, max_misses=3, tentative_misses=0,
                   max_candidates=L.RTS_TRACK_MAX_CAND, max_tracks=0, device_plots=None, n_plots=0, fetch=True):
        """rts_cube_track + rts_cube_tracks_get: the handle's track table advanced by the frame at `time` -- the handle's plots
        (device_plots None) or a caller-owned device array of n_plots RtsPlot records; sigma is the measurement standard deviation
        (delay in s, Doppler in Hz).  Never waits on the host unless fetch.  Returns (the TRACK_DTYPE table, next_id) when fetch."""
        p = _track_params(gate, sigma, q, delay_rate_per_hz, doppler_period, confirm_hits, max_misses, tentative_misses, max_candidates, max_tracks,
                          device_plots, n_plots)
        check(L.lib().rts_cube_track(self.h, C.byref(p), float(time)))
        return self.tracks() if fetch else None

    def tracks(self):
        """rts_cube_tracks_get: (the stored tracks, next_id); raises when a full table turned new tracks away"""
        n, nid = C.c_uint32(0), C.c_uint64(0)
        rc = L.lib().rts_cube_tracks_get(self.h, None, 0, C.byref(n), C.byref(nid))
        if rc not in (L.RTS_OK, L.RTS_ERR_CAPACITY):
            check(rc)
        out = np.zeros(max(n.value, 1), L.TRACK_DTYPE)
        check(L.lib().rts_cube_tracks_get(self.h, ptr(out), n.value, C.byref(n), C.byref(nid)))
        return out[:n.value].copy(), nid.value

    def cube_tracks_set(self, tracks, next_id, time):
        """rts_cube_tracks_set: loads a TRACK_DTYPE table, the next id and the time the tracks stand at (waits for the handle's stream)"""
        t = np.ascontiguousarray(np.asarray(tracks, L.TRACK_DTYPE))
        check(L.lib().rts_cube_tracks_set(self.h, ptr(t) if len(t) else None, len(t), int(next_id), float(time)))

    def cube_tracks_reset(self):
        """rts_cube_tracks_reset: an empty table without a time; ids go on where they were"""
        check(L.lib().rts_cube_tracks_reset(self.h))

    def cube_locate(self, tx, rx_positions, cspeed, carrier, sigma, gate=9.21, assoc_delay=1e-7, box=((-1e6,) * 3, (1e6,) * 3), anchors=(0, 1, 2),
                    min_receivers=None, n_iters=4, max_candidates=0, max_targets=0, source="plots", device_list=None, n_list=0, fetch=True):
        """rts_cube_locate + rts_cube_targets_get: one frame of per-receiver records -- the handle's plots or its track table (source
        "plots" / "tracks", device_list None), a caller-owned device array of n_list RtsPlot records, or for the resolution alone n_list
        RtsTarget candidates (source "candidates") -- to targets: position, velocity and the records they are made of, seen from a
        transmitter at tx by the receivers at rx_positions [n_rx][3]; sigma is the measurement standard deviation (delay in s, Doppler
        in Hz).  Never waits on the host unless fetch.  Returns a TARGET_DTYPE array in ascending candidate index when fetch."""
        p, keep = _locate_params(tx, rx_positions, cspeed, carrier, sigma, gate, assoc_delay, box, anchors, min_receivers, n_iters, max_candidates, max_targets,
                                 source, device_list, n_list)
        check(L.lib().rts_cube_locate(self.h, C.byref(p)))
        return self.cube_targets() if fetch else None

    def cube_targets(self):
        """rts_cube_targets_get: the targets of the last cube_locate (every stored record; raises when a capacity cut them)"""
        n = C.c_uint32(0)
        rc = L.lib().rts_cube_targets_get(self.h, None, 0, C.byref(n))
        if rc not in (L.RTS_OK, L.RTS_ERR_CAPACITY):
            check(rc)
        out = np.zeros(max(n.value, 1), L.TARGET_DTYPE)
        check(L.lib().rts_cube_targets_get(self.h, ptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def cube_tbd_step(self, time, half=(1, 2), depth=8, score="power", scale=1.0, decay=1.0, delay_rate_per_hz=0.0, pri=0.0, device_ptr=None, n_doppler=0):
        """rts_cube_tbd_step: the handle's track-before-detect state advanced by the frame at `time` -- the handle's last cube_doppler
        map (device_ptr None) or a caller complex128 device map [n_rx][n_doppler][n_bins]; half is the transition window (Doppler,
        range) in cells on each side; scale is 1 / noise power.  Never waits on the host."""
        p = _tbd_params(half, depth, score, scale, decay, delay_rate_per_hz, pri)
        check(L.lib().rts_cube_tbd_step(self.h, C.byref(p), float(time), C.c_void_p(device_ptr) if device_ptr else None, int(n_doppler or 0)))
        self._tbd_pri = float(pri)

    def cube_tbd_extract(self, threshold, local_max=True, max_tracks=0, fetch=True, pri=None):
        """rts_cube_tbd_extract + the getters: the cells of the merit map above `threshold` (local_max: only 3 x 3 local maxima), each
        walked back through the pointer ring; pri (None: the last cube_tbd_step's) turns doppler_bin into hertz.  Never waits on the
        host unless fetch.  Returns (the TBD_TRACK_DTYPE records, their paths uint32 [n][depth][2]) when fetch."""
        e = _tbd_extract_params(threshold, local_max, max_tracks, getattr(self, "_tbd_pri", 0.0) if pri is None else pri)
        check(L.lib().rts_cube_tbd_extract(self.h, C.byref(e)))
        return self.tbd_tracks() if fetch else None

    def tbd_info(self):
        """rts_cube_tbd_info: ((n_rx, n_doppler, n_bins, depth), frames) of the track-before-detect state; zeros without one"""
        shape, frames = (C.c_uint32 * 4)(), C.c_uint64(0)
        check(L.lib().rts_cube_tbd_info(self.h, C.byref(shape), C.byref(frames)))
        return tuple(shape), frames.value

    def tbd_tracks(self):
        """rts_cube_tbd_tracks_get + rts_cube_tbd_paths_get: (records, paths) of the last cube_tbd_extract (every stored record; raises
        when max_tracks cut them)"""
        n = C.c_uint32(0)
        rc = L.lib().rts_cube_tbd_tracks_get(self.h, None, 0, C.byref(n))
        if rc not in (L.RTS_OK, L.RTS_ERR_CAPACITY):
            check(rc)
        depth = self.tbd_info()[0][3]
        out = np.zeros(max(n.value, 1), L.TBD_TRACK_DTYPE); paths = np.zeros((max(n.value, 1), max(depth, 1), 2), np.uint32)
        check(L.lib().rts_cube_tbd_tracks_get(self.h, ptr(out), n.value, C.byref(n)))
        check(L.lib().rts_cube_tbd_paths_get(self.h, ptr(paths), n.value))
        return out[:n.value].copy(), paths[:n.value].copy()

    def tbd_merit(self):
        """rts_cube_tbd_merit_get: the merit map, f64 [n_rx][n_doppler][n_bins]"""
        (n_rx, nd, nb, _), _ = self.tbd_info()
        out = np.zeros((max(n_rx, 1), max(nd, 1), max(nb, 1)))
        check(L.lib().rts_cube_tbd_merit_get(self.h, ptr(out), out.size))
        return out

    def tbd_ring(self):
        """rts_cube_tbd_ring_get: (the stored pointer maps uint8 [n][n_rx][n_doppler][n_bins], their shift tables int32 [n][n_doppler]),
        oldest first, n = min(frames, depth)"""
        (n_rx, nd, nb, depth), frames = self.tbd_info()
        n = C.c_uint32(0); k = max(min(frames, depth), 1)
        codes = np.zeros((k, max(n_rx, 1), max(nd, 1), max(nb, 1)), np.uint8); shifts = np.zeros((k, max(nd, 1)), np.int32)
        check(L.lib().rts_cube_tbd_ring_get(self.h, ptr(codes), ptr(shifts), k, C.byref(n)))
        return codes[:n.value], shifts[:n.value]

    def cube_tbd_reset(self):
        """rts_cube_tbd_reset: ends the track-before-detect state and its extraction; the next cube_tbd_step fixes shape and window anew"""
        check(L.lib().rts_cube_tbd_reset(self.h))

    def cube_backproject(self, origin, step_x, step_y, n_x, n_y, tx_positions, rx_positions, cspeed, carrier, taps=8, first=0, count=None,
                         weights=None, accumulate=False, device_ptr=None, fetch=True):
        """rts_cube_backproject: the attached cube's rows first .. first + count - 1 backprojected onto the pixel grid origin + ix step_x +
        iy step_y; tx_positions [count][3], rx_positions [n_rx][count][3] in the image's frame (image_frame for ISAR).  Into a caller
        complex128 device tensor [n_rx][n_y][n_x] (device_ptr; nothing is fetched) or the library's image, returned complex
        [n_rx][n_y][n_x] when fetch"""
        p, keep = _image_params(origin, step_x, step_y, n_x, n_y, tx_positions, rx_positions, cspeed, carrier, taps, first, count, weights, accumulate,
                                self._cube_shape[0])
        check(L.lib().rts_cube_backproject(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._image_shape = (self._cube_shape[0], int(n_y), int(n_x))
        return self.image() if fetch else None

    def image(self):
        """rts_cube_image_get: the library-owned image of the last cube_backproject"""
        shape = getattr(self, "_image_shape", None) or (1, 1, 1)
        out = np.zeros(shape + (2,), np.float64)
        check(L.lib().rts_cube_image_get(self.h, ptr(out), out.size))
        return out[..., 0] + 1j * out[..., 1]

    def cube_spectrogram(self, window_len, hop, n_fft, window=None, first=0, count=None, first_bin=0, n_bins=0, power=False, sum_bins=False,
                         device_ptr=None, fetch=True):
        """rts_cube_spectrogram: the short-time Fourier transform over the pulse axis of the attached cube's rows first .. first + count - 1
        (default: to the last), frames of window_len pulses every hop pulses, tapered by window (an array of window_len values, or
        None), zero-padded to n_fft, for the gate first_bin .. first_bin + n_bins - 1 (n_bins 0: to the last bin).  Into a caller
        device tensor (device_ptr; nothing is fetched) or the library's output, returned when fetch: complex
        [n_rx][n_frames][n_fft][n_gate], float64 of that shape with power, float64 [n_rx][n_frames][n_fft] with power and sum_bins"""
        n_rx, n_p, nb = self._cube_shape
        p, keep = _stft_params(window_len, hop, n_fft, window, first, count, first_bin, n_bins, power, sum_bins, n_p)
        nf = C.c_uint32(0)
        check(L.lib().rts_cube_spectrogram(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None, C.byref(nf)))
        if device_ptr:
            return None
        self._stft_shape = _stft_shape(n_rx, nf.value, p.n_fft, p.n_bins if p.n_bins else nb - p.first_bin, power, sum_bins)
        return self.spectrogram() if fetch else None

    def spectrogram(self):
        """rts_cube_spectrogram_get: the library-owned output of the last cube_spectrogram"""
        shape, dtype = getattr(self, "_stft_shape", None) or ((1, 1, 2), np.float64)
        out = np.zeros(shape, dtype)
        check(L.lib().rts_cube_spectrogram_get(self.h, ptr(out), out.size * (2 if dtype is np.complex128 else 1)))
        return out

    def cube_align(self, first=0, count=None, gate=None, max_lag=8, n_iters=4, integer=False, device_ptr=None, fetch=True):
        """rts_cube_align: the range shifts of the attached cube's rows first .. first + count - 1 (default: to the last) against their
        global reference, over the gate (None: the whole row, or (first_bin, n_gate)), lags up to max_lag (it must cover the whole
        walk).  Into a caller float64 device tensor [n_rx][count] (device_ptr; nothing is fetched) or the handle's shift table,
        returned float64 [n_rx][count] when fetch"""
        n_rx, n_p, nb = self._cube_shape
        p = _align_params(first, count, gate, max_lag, n_iters, integer, n_p)
        check(L.lib().rts_cube_align(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._align_shape = (n_rx, p.n_pulses)
        return self.align_shifts() if fetch else None

    def align_shifts(self):
        """rts_cube_align_get: the handle's shift table"""
        out = np.zeros(getattr(self, "_align_shape", None) or (1, 1))
        check(L.lib().rts_cube_align_get(self.h, ptr(out), out.size))
        return out

    def cube_pga(self, first=0, count=None, gate=None, n_iters=6, window0=0, window_min=0, device_ptr=None, fetch=True):
        """rts_cube_pga: the phase error of rows first .. first + count - 1 (count a power of two in [4, 4096]) by phase-gradient
        autofocus over the gate; the cube is not changed.  Into a caller float64 device tensor of n_rx (count + n_iters) values
        (device_ptr: the phase [n_rx][count], then the rms [n_rx][n_iters]; nothing is fetched) or the handle's phase table, returned
        (phase in cycles [n_rx][count], rms [n_rx][n_iters]) when fetch"""
        n_rx, n_p, nb = self._cube_shape
        p = _pga_params(first, count, gate, n_iters, window0, window_min, n_p)
        check(L.lib().rts_cube_pga(self.h, C.byref(p), C.c_void_p(device_ptr) if device_ptr else None))
        if device_ptr:
            return None
        self._pga_shape = (n_rx, p.n_pulses, p.n_iters)
        return self.pga_phase() if fetch else None

    def pga_phase(self):
        """rts_cube_pga_get: (the handle's phase table, its convergence record)"""
        n_rx, n, it = getattr(self, "_pga_shape", None) or (1, 1, 1)
        phase = np.zeros((n_rx, n)); rms = np.zeros((n_rx, it))
        check(L.lib().rts_cube_pga_get(self.h, ptr(phase), ptr(rms), phase.size, rms.size))
        return phase, rms

    def cube_correct(self, shifts=None, phase=None, first=0, count=None, taps=8, use_align=False, use_pga=False):
        """rts_cube_correct: rows first .. first + count - 1 of the attached cube resampled at n + shifts (bins) and rotated by -phase
        (cycles), in place; shifts, phase: host arrays [n_rx][count], or use_align / use_pga: the handle's tables, on the device"""
        n_rx, n_p, nb = self._cube_shape
        p, keep = _correct_params(first, count, taps, shifts, phase, use_align, use_pga, n_rx, n_p)
        check(L.lib().rts_cube_correct(self.h, C.byref(p)))

    def cube_autofocus(self, first=0, count=None, gate=None, max_lag=8, taps=8, align_iters=4, **pga_kwargs):
        """align -> correct(shifts) -> pga -> correct(phase) on the attached cube, nothing fetched in between; pga_kwargs: n_iters,
        window0, window_min.  Returns (shifts [n_rx][count], phase [n_rx][count], rms [n_rx][n_iters])"""
        self.cube_align(first, count, gate, max_lag, align_iters, fetch=False)
        self.cube_correct(first=first, count=count, taps=taps, use_align=True)
        self.cube_pga(first, count, gate, fetch=False, **pga_kwargs)
        self.cube_correct(first=first, count=count, taps=taps, use_pga=True)
        phase, rms = self.pga_phase()
        return self.align_shifts(), phase, rms

    def cube(self):
        out = np.zeros(self._cube_shape + (2,), np.float64)
        check(L.lib().rts_cube_get(self.h, ptr(out), out.size))
        return out[..., 0] + 1j * out[..., 1]

    def bvh(self):
        """static target-space hierarchy: (nodes [n][32] float32 view of the 128-byte records, leaf_prim, roots)"""
        s = self.scene_info()                                                         # (the scene's records: stats() holds those of the last finished launch's scene)
        nl = C.c_uint32(0)
        check(L.lib().rts_get_bvh(self.h, None, None, None, 0, 0, C.byref(nl)))        # leaf slots (>= primitives: split references)
        nodes = np.zeros((max(s["n_nodes"], 1), 32), np.float32); leaf = np.zeros(max(nl.value, 1), np.uint32)
        roots = np.zeros(max(self.n_targets, 1), np.int32)
        check(L.lib().rts_get_bvh(self.h, ptr(nodes), ptr(leaf), ptr(roots), nodes.shape[0], leaf.shape[0], C.byref(nl)))
        return nodes[:s["n_nodes"]], leaf[:nl.value], roots[:self.n_targets]

    def self_test_math(self, y, x, a, b):
        y = np.ascontiguousarray(y, np.float32); x = np.ascontiguousarray(x, np.float32)
        a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
        n = len(y); at = np.zeros(n, np.float32); dv = np.zeros(n); sq = np.zeros(n)
        check(L.lib().rts_self_test_math(self.h, ptr(y), ptr(x), ptr(at), ptr(a), ptr(b), ptr(dv), ptr(sq), n))
        return at, dv, sq
