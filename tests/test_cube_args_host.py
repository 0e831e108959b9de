"""The pure argument rules of the cube entry points (rts_amd/csrc/rts_cube_args.h) without a GPU and without HIP: a span inside a
total, a power of two in a range, byte ranges against each other, an output against every receiver's span of the input, the
source fields of a beamformer-style record, a counted list's copied count.  tests/cube_args/cube_args_main.cpp includes the header
alone and is built with g++ (under AddressSanitizer + UndefinedBehaviorSanitizer where g++ has them).  The addresses are integers:
no memory is touched.  Every expectation is written out or restated here in Python."""
import itertools

import pytest

import helpers as H

CELL = 16                            # one complex128
FROM_CUBE, FROM_MAP, FROM_POINTER = 0, 1, 2      # RTS_BEAM_FROM_* (include/rts_amd.h)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    run = H.host_driver(tmp_path_factory, "cube_args/cube_args_main.cpp")

    def ask(lines):
        out = run("".join(" ".join(str(int(x)) if not isinstance(x, str) else x for x in ln) + "\n" for ln in lines)).split("\n")[:-1]
        assert len(out) == len(lines)
        return [[int(x) for x in ln.split()] for ln in out]
    return ask


# ---------------------------------------------------------------------------------------------- output against the receivers' spans
SRC, STRIDE, CELL0 = 0x7f0000100000, 40, 8      # the source's base; cells per receiver; the first cell read (first_row > 0: a gap in front of every span)


def span_bytes(r, cell0=CELL0, cell1=CELL0 + 1):
    return SRC + CELL * (r * STRIDE + cell0), SRC + CELL * (r * STRIDE + cell1)


def rx_case(out0, out1, n_rx, cell0=CELL0, cell1=CELL0 + 1):
    return ("rx", out0, out1 - out0, SRC, STRIDE, cell0, cell1, n_rx)


@pytest.mark.parametrize("n_rx", [1, 2, 64])
def test_overlap_accepts_what_touches_a_span_and_refuses_one_cell_inside(ask, n_rx):
    cases, want = [], []
    for r in sorted({0, n_rx - 1}):
        i0, i1 = span_bytes(r)
        # accepted: the output ends exactly at the span's first byte; begins exactly at its one-past-last byte; lies in the gap in front of it
        cases += [rx_case(i0 - 2 * CELL, i0, n_rx), rx_case(i1, i1 + 2 * CELL, n_rx), rx_case(i0 - CELL0 * CELL, i0 - CELL, n_rx)]
        want += [[0, -1]] * 3
        if r + 1 < n_rx:             # ... in the gap between this receiver's span and the next one's, all of it
            cases.append(rx_case(i1, span_bytes(r + 1)[0], n_rx)); want.append([0, -1])
        # refused: one cell into the span from below, from above, the whole span covered, exactly the span
        cases += [rx_case(i0 - CELL, i0 + CELL, n_rx), rx_case(i1 - CELL, i1 + CELL, n_rx), rx_case(i0 - CELL, i1 + CELL, n_rx), rx_case(i0, i1, n_rx)]
        want += [[1, r]] * 4
        # one byte is an overlap too
        cases += [rx_case(i0 - CELL, i0 + 1, n_rx), rx_case(i1 - 1, i1 + CELL, n_rx)]
        want += [[1, r]] * 2
    assert ask(cases) == want


@pytest.mark.parametrize("n_rx", [2, 64])
def test_overlap_reports_the_first_receiver(ask, n_rx):
    last = n_rx - 1
    everything = rx_case(SRC, span_bytes(last)[1], n_rx)                      # covers every span: receiver 0
    from_one_on = rx_case(span_bytes(0)[1], span_bytes(last)[1], n_rx)          # begins behind receiver 0's span: receiver 1
    behind_all = rx_case(span_bytes(last)[1], span_bytes(last)[1] + 4096, n_rx)
    fewer = rx_case(span_bytes(last)[0], span_bytes(last)[1], n_rx - 1)         # the last receiver's span is not read by a call over n_rx - 1
    assert ask([everything, from_one_on, behind_all, fewer]) == [[1, 0], [1, 1], [0, -1], [0, -1]]


def test_overlap_spans_of_several_cells_and_none(ask):
    i0, i1 = span_bytes(1, 3, 9)
    assert ask([rx_case(i0 - CELL, i0, 2, 3, 9), rx_case(i1 - CELL, i1, 2, 3, 9), rx_case(i1, i1 + CELL, 2, 3, 9), rx_case(i0, i1, 0, 3, 9)]) == [[0, -1], [1, 1], [0, -1], [0, -1]]


def test_bytes_overlap(ask):
    a = 0x1000
    cases = [("bytes", a, 32, a + 32, 16), ("bytes", a + 32, 16, a, 32), ("bytes", a, 32, a + 31, 16), ("bytes", a + 31, 16, a, 32),
             ("bytes", a, 64, a + 16, 16), ("bytes", a + 16, 16, a, 64), ("bytes", a, 16, a, 16), ("bytes", a, 0, a, 16)]
    assert ask(cases) == [[0], [0], [1], [1], [1], [1], [1], [0]]


# ---------------------------------------------------------------------------------------------- spans, powers of two, counts
def span_restated(first, n, total, zero_to_end, at_least_one):
    if first >= total or first + n > total:          # (Python's integers do not wrap)
        return [0, 0]
    count = total - first if (n == 0 and zero_to_end) else n
    return [0, 0] if (at_least_one and count == 0) else [1, count]


def test_span_at_its_edges(ask):
    total = 8
    spans = [(total, 0), (total, 1), (total - 1, 1), (3, total - 3), (3, total - 3 + 1), (0, total), (0, total + 1), (2, 0xffffffff), (0xffffffff, 2), (0, 0), (3, 0), (0, 1)]
    cases, want = [], []
    for (first, n), zero_to_end, at_least_one in itertools.product(spans, (0, 1), (0, 1)):
        cases.append(("span", first, n, total, zero_to_end, at_least_one)); want.append(span_restated(first, n, total, zero_to_end, at_least_one))
    got = ask(cases)
    assert got == want
    by = {c[1:]: g for c, g in zip(cases, got)}
    assert by[(total, 0, total, 1, 0)] == [0, 0]                 # first == total is outside, whatever n == 0 means
    assert by[(3, total - 3, total, 0, 1)] == [1, total - 3]       # n == total - first: the last element is in
    assert by[(3, total - 3 + 1, total, 0, 0)] == [0, 0]         # ... one more is out
    assert by[(2, 0xffffffff, total, 0, 0)] == [0, 0]            # first + n wraps to 1: still outside
    assert by[(3, 0, total, 1, 1)] == [1, total - 3]             # n == 0: to the end ...
    assert by[(3, 0, total, 0, 0)] == [1, 0]                     # ... or a span of none, which is inside ...
    assert by[(3, 0, total, 0, 1)] == [0, 0]                     # ... and refused where at least one is required


def test_span_of_an_empty_total(ask):
    assert ask([("span", 0, 0, 0, 1, 0), ("span", 0, 0, 0, 0, 0)]) == [[0, 0], [0, 0]]


@pytest.mark.parametrize("lo,hi", [(2, 4096), (4, 1024), (2, 0x80000000)])
def test_power_of_two_in_a_range(ask, lo, hi):
    values = [0, 1, 2, 3, 4, lo, lo - 1, hi - 1, hi, hi + 1, (2 * hi) & 0xffffffff, 0xffffffff]
    want = [[1 if (v >= lo and v <= hi and v > 0 and bin(v).count("1") == 1) else 0] for v in values]
    got = ask([("pow2", v, lo, hi) for v in values])
    assert got == want
    assert got[values.index(hi)] == [1] and got[values.index(0)] == [0] and got[values.index(3)] == [0] and got[values.index(1)] == [0]
    assert got[values.index((2 * hi) & 0xffffffff)] == [0]


def test_copied_count_of_a_list(ask):
    cases = [(t, m, c) for t in (0, 1, 5, 0xffffffff) for m in (0, 4, 5, 0xffffffff) for c in (0, 3, 5, 0xffffffff)]
    assert ask([("copied",) + c for c in cases]) == [[min(c)] for c in cases]


# ---------------------------------------------------------------------------------------------- the record's source fields
def source_lines_restated(source, n_rows_in, device_in):
    """the four lines the rule replaces, in their order (rts_beam_check, rts_cov_check, rts_st_apply_check)"""
    if source > FROM_POINTER:
        return 1          # unknown source %u (RTS_BEAM_FROM_CUBE, _MAP, _POINTER)
    if source != FROM_POINTER and n_rows_in != 0:
        return 2          # n_rows_in = %u without RTS_BEAM_FROM_POINTER
    if source != FROM_POINTER and device_in:
        return 3          # device_in without RTS_BEAM_FROM_POINTER
    if source == FROM_POINTER and n_rows_in == 0:
        return 4          # n_rows_in = 0 with RTS_BEAM_FROM_POINTER
    return 0


def test_source_fields_rule_on_every_combination(ask):
    combos = list(itertools.product((0, 1, 2, 3), (0, 4), (0, 1)))
    got = ask([("source",) + c for c in combos])
    assert got == [[source_lines_restated(*c)] for c in combos]
    by = dict(zip(combos, (g[0] for g in got)))
    assert by[(3, 4, 1)] == 1 and by[(0, 4, 1)] == 2 and by[(1, 0, 1)] == 3 and by[(2, 0, 1)] == 4      # several wrong fields: the first rule in the lines' order
    assert by[(0, 0, 0)] == by[(1, 0, 0)] == by[(2, 4, 1)] == by[(2, 4, 0)] == 0                           # (a null device_in with _POINTER is the resolver's to refuse)
