"""CPU: the guards of tests/kernel_code_cases.py (the inputs of tests/test_gpu_kernel_codes.py).  Every case is a well-defined input of
every kernel, reaches the plan it is listed for under the library's own host arithmetic, its float64 restatement stands against the long
double reference, and the parity tests bite: bytes read as unsigned in one place move every centred kernel by 1e-3 or more.

Measured here, restatement against long double (scaled_err): EigenGRM(True) 3.1e-12, GRM 2.9e-12 (both flags), EigenARC(True) 2.0e-12,
all on tpod100 (the identity's cancellation, 2^-53 max|G| / max|ZZ'|); pair GAU 7.9e-15 (pair_mixed: exp of a large exponent), pair ARC
6.0e-16; every other case and kind at or below 1e-15.  The smallest movement under a misread byte is 2.2e-2 (full3, EigenARC(True), the
row sums)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels_restatement as KR   # noqa: E402
import kernel_code_cases as KC   # noqa: E402

LD_BOUND = 1e-9      # against the long double reference: the bound of the PEGS codes tests for the same kind of comparison, a factor of
                     # about 300 over the identity's own cancellation on tpod100 (2^-53 x 3e4 = 3e-12) and 1e6 below a misread byte
BITE = 1e-3
KS = range(len(KR.KINDS))


def _dup_pairs(X):
    """unordered pairs of equal rows"""
    G = KR.crossprod(X)
    d = np.diag(G)
    d2 = d[:, None] + d[None, :] - 2 * G
    return [(i, j) for i, j in zip(*np.nonzero(d2 == 0)) if i < j]


def test_the_gram_bound_holds_and_the_codes_are_what_the_table_says():
    want = {"pm1": (196, 376, -1, 1), "tpod100": (196, 376, 100, 102), "full": (300, 200, -128, 127), "full3": (700, 900, -128, 127),
            "pm127": (257, 129, -127, 127), "dos100": (130, 65, 0, 100), "hold_dup": (300, 200, -128, 127), "n2": (2, 63, -128, 127),
            "n3p1": (3, 1, -128, 127), "n129p1": (129, 1, -3, 3), "n130p63": (130, 63, -3, 3), "n257p65": (257, 65, -3, 3)}
    assert sorted(want) == sorted(KC.TAGS)
    for tag in KC.TAGS:
        X = KC.data(tag)
        assert X.dtype == np.int8 and not X.flags.writeable
        if tag == "n2":      # two rows of 63 draws need not reach the ends of the range
            assert X.shape == (2, 63) and X.min() < -100 and X.max() > 100
        else:
            assert (X.shape[0], X.shape[1], int(X.min()), int(X.max())) == want[tag], tag
        assert X.shape[0] * KC.xmax(X) ** 2 < 2 ** 31, tag
    assert set(np.unique(KC.data("pm127"))) == {-127, 127}
    H = KC.data("hold_dup")
    assert np.all(H[:, 5] == -128) and np.all(H[:, 9] == 127) and np.array_equal(H[7], H[3])
    assert np.array_equal(KC.data("pm1").astype(int) + 1, KC.data("tpod")) and np.array_equal(KC.data("tpod100").astype(int) - 100, KC.data("tpod"))
    shapes = {"pair_pm1": (130, 66, 376), "pair_full": (300, 170, 200), "pair_mixed": (300, 170, 200), "pair_slabs": (700, 300, 900), "pair_ns2": (300, 2, 200)}
    for tag, (nf, ns, p) in shapes.items():
        F, S = KC.pair_data(tag)[:2]
        assert F.shape == (nf, p) and S.shape == (ns, p), tag
        Fs, Ss = KC.pair_data(tag, True)[:2]
        assert Fs is S and Ss is F
    assert np.all(KC.pair_data("pair_full")[1][7] == -128)
    F, S = KC.pair_data("pair_mixed")[:2]
    assert (F.min(), F.max(), S.min(), S.max()) == (0, 2, -128, 127)


def test_duplicate_rows_are_where_the_table_puts_them():
    """hold_dup has exactly one off-diagonal pair at distance 0, rows 3 and 7.  n129p1 has one marker with seven codes over 129 rows, so
    its rows repeat by counting alone (GAU and EigenGAU meet exact zero distances there too).  No other case has a duplicate row."""
    for tag in KC.TAGS:
        dup = _dup_pairs(KC.data(tag))
        if tag == "hold_dup":
            assert dup == [(3, 7)]
        elif tag == "n129p1":
            assert len(np.unique(KC.data(tag))) == 7 and len(dup) > 0
        else:
            assert dup == [], (tag, dup[:3])
    for tag, swapped in KC.ORIENTATIONS:
        F = KC.pair_data(tag, swapped)[0]
        assert _dup_pairs(F) == [], (tag, swapped)


def test_every_case_is_a_well_defined_input():
    """Finite restatements, acos arguments inside the slack, D, md and the mean diagonal > 0.  The one exception is the reference's own:
    the uncentred EigenARC is 0 / 0 on a row of zeros, which only n129p1 has (x = 0 at its one marker); the restatement and the long double
    reference are not-a-number on exactly those rows and columns, and the GPU test asserts the same mask of the library."""
    for tag in KC.TAGS:
        X = KC.data(tag)
        n = X.shape[0]
        assert bool(KC.zero_rows(X).any()) == (tag == "n129p1"), tag
        for k in KS:
            K, mask = KC.restated(tag, k), KC.undefined(tag, k)
            assert K.shape == (n, n) and np.array_equal(np.isfinite(K), ~mask), (tag, KC.kind_id(k))
            assert np.array_equal(np.isfinite(KC.reference(tag, k).astype(np.float64)), ~mask), (tag, KC.kind_id(k))
            assert mask.any() == (tag == "n129p1" and KC.kind_id(k) == "EigenARC-False")
            assert np.array_equal(K, K.T, equal_nan=True)
            if KR.KINDS[k][0] in ("GAU", "EigenGAU"):
                assert np.array_equal(np.diag(K), np.ones(n))
        for cen in (True, False):
            arg = KC.arc_argument(tag, cen)
            assert arg <= 1.0 / np.sqrt(1.001) + 1e-12, (tag, cen, arg)
        Xi = X.astype(np.int64)
        s, q = Xi.sum(0).astype(np.float64), (Xi * Xi).sum(0).astype(np.float64)
        assert np.sum((q - s * s / n) / (n - 1.0)) > 0 and np.sum((s / n) ** 2 / 2.0) > 0, tag        # GRM's two D
        G = KR.crossprod(X)
        d = np.diag(G)
        assert (d[:, None] + d[None, :] - 2 * G).sum() > 0, tag                                          # GAU's md, EigenGAU's sum
        assert np.mean(np.diag(KR.zz_identity(X))) > 0 and np.mean(d) > 0, tag                          # the mean diagonals
    for tag, swapped in KC.ORIENTATIONS:
        for kind, phi in KC.PAIR_KINDS:
            for K in KC.restated2(tag, swapped, kind, phi):
                assert np.all(np.isfinite(K)), (tag, swapped, kind)
        F, S = KC.pair_data(tag, swapped)[:2]
        Aff, Afs, ds = KC.K2.arc_centred_direct(F, S)
        df = np.diag(Aff)
        assert df.min() > 0 and ds.min() > 0
        assert np.abs(Afs / np.sqrt(df[:, None] * ds[None, :] * 1.001)).max() <= 1.0 / np.sqrt(1.001) + 1e-12


def test_every_case_reaches_the_plan_it_is_listed_for():
    pl = {tag: KC.panel_plan(KC.data(tag), KC.CASES[tag]["kw"]) for tag in KC.TAGS}
    assert (pl["full3"]["K"], pl["full3"]["R"], pl["full3"]["ld"]) == (3, 256, 768)
    xp = KC.xxt_plan(KC.data("full3"))
    assert xp["nchunks"] == 1 and xp["chunk"] == (2 ** 31 - 1) // 128 ** 2 and xp["T"] == 6
    assert 900 % 64 == 4                                                         # the partial last block
    for kchunk, chunks in ((64, 15), (100, 9)):                                  # BWGR_KCHUNK of the GPU test
        assert KC.xxt_plan(KC.data("full3"), kchunk)["nchunks"] == chunks
    for tag in KC.TAGS:
        X = KC.data(tag)
        rows, colwg = KC.rows_grid(pl[tag]["ld"], X.shape[1])
        assert rows == pl[tag]["ld"] // 128 >= 1
        if tag in ("n3p1", "n129p1"):
            assert colwg == 1 and (X.shape[1] + 3) // 4 == 1                     # one column workgroup; one workgroup of k_kfin_colstats
        assert KC.xxt_plan(X)["T"] == -(-X.shape[0] // 128)
    assert pl["pm127"]["ld"] >= 384 and pl["n257p65"]["ld"] >= 384               # three row workgroups: one past two blocks of 128
    F, S, kwf, kws = KC.pair_data("pair_slabs")
    pf, ps = KC.panel_plan(F, kwf), KC.panel_plan(S, kws)
    print("pair_slabs: founders", pf, "samples", ps)
    assert (pf["K"], pf["R"]) == (3, 256) and (ps["K"], ps["R"]) == (3, 128)
    yp = KC.xyt_plan(F, S)
    assert yp["nchunks"] == 1 and (yp["Tr"], yp["Tc"]) == (6, 3)
    F, S = KC.pair_data("pair_mixed")[:2]
    assert KC.xyt_plan(F, S)["chunk"] == (2 ** 31 - 1) // (2 * 128)              # each panel's own largest |x|
    F, S, kwf, kws = KC.pair_data("pair_pm1")
    assert KC.panel_plan(F, kwf)["R"] != KC.panel_plan(S, kws)["R"]             # the tpod split: one slab of 256 against one of 128


def test_the_restatement_stands_against_the_long_double_reference():
    worst = {}
    for tag in KC.TAGS:
        for k in KS:
            e = KC.err(KC.restated(tag, k), KC.reference(tag, k), KC.undefined(tag, k))
            print("%-8s %-16s restatement against long double: %.3e" % (tag, KC.kind_id(k), e))
            worst[KC.kind_id(k)] = max(worst.get(KC.kind_id(k), (0.0, "")), (e, tag))
            assert e <= LD_BOUND, (tag, KC.kind_id(k), e)
    for tag, swapped in KC.ORIENTATIONS:
        for kind, phi in KC.PAIR_KINDS:
            es = [KC.err(a, b) for a, b in zip(KC.restated2(tag, swapped, kind, phi), KC.reference2(tag, swapped, kind, phi))]
            print("%-10s %-7s %s phi=%s: Kff %.3e, Kfs %.3e" % (tag, "swapped" if swapped else "", kind, phi, es[0], es[1]))
            key = "pair %s" % kind
            worst[key] = max(worst.get(key, (0.0, "")), (max(es), tag + ("/swapped" if swapped else "")))
            assert max(es) <= LD_BOUND, (tag, swapped, kind, phi, es)
    for key, (e, tag) in worst.items():
        print("worst %-16s %.3e on %s" % (key, e, tag))


def test_the_shifted_panels_share_one_centred_kernel():
    """X - mean is the same matrix on pm1, tpod and tpod100: the long double references of the centred kinds agree to long double's own
    rounding, which is what makes the GPU's library-against-library comparison a check of the identity alone."""
    for k in KS:
        if not KC.centred_kind(k):
            continue
        for a in KC.SHIFTED:
            e = KC.err(KC.reference(a, k).astype(np.float64), KC.reference("tpod", k))
            print("%-16s %s against tpod, long double: %.3e" % (KC.kind_id(k), a, e))
            assert e <= 1e-15, (KC.kind_id(k), a, e)


def test_the_tests_bite():
    """A byte read as unsigned in one place only -- the column sums s, the row sums X s, the samples' row squares q_s -- moves each centred
    kernel of each case with negative codes by at least 1e-3: six orders above the long double bound, three above the parity bound."""
    smallest = (np.inf, "")
    signed = [tag for tag in KC.TAGS if KC.has_negative(KC.data(tag))]
    assert signed == [tag for tag in KC.TAGS if tag not in ("tpod100", "dos100")]
    for tag in signed:
        X = KC.data(tag)
        for k in KS:
            if not KC.uses_sums(k):
                continue
            for where in ("s", "Xs"):
                mask = KC.undefined(tag, k)
                m = KC.moved(KC.misread(k, tag, where)[~mask], KC.restated(tag, k)[~mask])
                print("%-8s %-16s %-2s read unsigned: moves by %.3e" % (tag, KC.kind_id(k), where, m))
                smallest = min(smallest, (m, "%s %s %s" % (tag, KC.kind_id(k), where)))
                assert m >= BITE, (tag, KC.kind_id(k), where, m)
    for tag, swapped in KC.ORIENTATIONS:
        F, S = KC.pair_data(tag, swapped)[:2]
        for where in KC.MISREADS:
            touched = KC.has_negative(S) if where == "qs" else (KC.has_negative(F) if where == "s" else KC.has_negative(F) or KC.has_negative(S))
            if not touched:
                continue
            for kind in ("ARC", "GAU") if where == "qs" else ("ARC",):
                got, ref = KC.misread2(kind, tag, swapped, where), KC.restated2(tag, swapped, kind, 1.0)
                m = KC.moved(got[1], ref[1]) if where == "qs" else max(KC.moved(got[0], ref[0]), KC.moved(got[1], ref[1]))
                print("%-10s %-7s pair %s %-2s read unsigned: moves by %.3e" % (tag, "swapped" if swapped else "", kind, where, m))
                smallest = min(smallest, (m, "%s%s pair %s %s" % (tag, "/swapped" if swapped else "", kind, where)))
                assert m >= BITE, (tag, swapped, kind, where, m)
    print("smallest movement under a misread byte: %.3e (%s)" % smallest)
    assert smallest[0] >= BITE


def test_the_long_double_reference_does_not_use_the_identity():
    import inspect
    src = inspect.getsource(KC.reference) + inspect.getsource(KC.reference2) + inspect.getsource(KC._ld_products)
    assert "identity" not in src
    assert np.finfo(KC.LD).eps <= 2.0 ** -63, "long double is no wider than double on this platform"
