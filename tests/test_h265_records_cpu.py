"""The record-level differential layer of the H.265 reconstruction (tests/_h265_records.py) on the CPU: the ctypes
mirrors against the C compiler, a lossless record / replay, the mutators' invariants and sensitivity, what the
committed seeds cover, and the domain cap.  tests/test_gpu_h265_records.py runs the same cases on gfx950.

Cases per family: len(STREAMS) x len(seeds(family)) = 15 (mv: 40).  With the committed seeds none is skipped by the domain rule (the
amplitudes are bounded by construction, see mutate_resid / mutate_flat), so the GPU test compares all of them."""
import numpy as np
import pytest

import _h265_records as R
from test_h265_cpu import GOLD, SMALL


def test_mirrors_match_c_layout(built):
    """sizeof / offsetof of h265r_tu_t, h265r_pu_t, h265r_sao_t, h265r_picture_t and h265r_backend_t as the C
    compiler lays them out (oracle/h265_oracle.c h265_oracle_layout) equal the ctypes mirrors'."""
    assert R.c_layout() == R.python_layout()
    assert (R.TU_DT.itemsize, R.PU_DT.itemsize, R.SAO_DT.itemsize) == (24, 16, 24)


@pytest.mark.parametrize("name", SMALL)
def test_record_replay_is_lossless(built, name):
    """Recorded, then replayed unmutated through the oracle: the snapshots hashed by frame_md5's rule in output
    order are the golden MD5s, with no domain violation."""
    rec, snaps, viol = R.case(None, name, 0)
    assert len(rec) == GOLD[name]["frames"]
    assert R.output_md5s(rec, snaps) == GOLD[name]["md5"]
    assert viol == 0


FIXED_TU = ("x", "y", "log2", "plane", "flags", "avail_top", "avail_left", "pad")


def _equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("family", R.FAMILIES)
def test_mutators_keep_the_structure(built, family):
    """Deterministic in the seed; geometry, record order, availability, the owner map and PU geometry untouched,
    field by field; each family changes only its own fields; the parent recording is never modified."""
    differs_by_seed = False
    for name in ("cov_h265_nosao_s1", "cov_h265_ldb_s1"):
        parent = R.recorded(name)
        before = parent.clone()
        a, b, c = R.MUTATORS[family](parent, 1), R.MUTATORS[family](parent, 1), R.MUTATORS[family](parent, 2)
        assert (a.n, a.width, a.height, a.output, a.geom) == (parent.n, parent.width, parent.height, parent.output, parent.geom)
        assert len(a) == len(b) == len(parent)
        differs_by_seed |= a.fill != c.fill
        for p0, p1, pa, pb, pc in zip(before, parent, a, b, c):
            for k in R.SCALARS:
                assert getattr(p0, k) == getattr(p1, k)
                assert getattr(pa, k) == getattr(pb, k)
            for k in R.ARRAYS:
                assert _equal(getattr(p0, k), getattr(p1, k)), "the parent recording was modified"
                assert _equal(getattr(pa, k), getattr(pb, k)), "not deterministic in the seed"
                differs_by_seed |= not _equal(getattr(pa, k), getattr(pc, k))
            differs_by_seed |= any(getattr(pa, k) != getattr(pc, k) for k in R.SCALARS)
            for k in ("width", "height", "pic_w", "pic_h", "ctb_log2", "slot"):
                assert getattr(pa, k) == getattr(p1, k)
            assert pa.n_tu == p1.n_tu and pa.n_pu == p1.n_pu and pa.n_coef >= p1.n_coef
            for f in FIXED_TU:
                assert np.array_equal(pa.tu[f], p1.tu[f]), f
            assert _equal(pa.map, p1.map)
            for f in ("x", "y", "w", "h"):
                assert np.array_equal(pa.pu[f], p1.pu[f]), f
            # bS bytes the parser left 0 stay 0
            assert not np.any((p1.bs_v == 0) & (pa.bs_v != 0)) and not np.any((p1.bs_h == 0) & (pa.bs_h != 0))
            # the domains both back ends read safely
            assert pa.tu["mode"].max(initial=0) <= 34 and pa.tu["res"].max(initial=0) <= 4
            assert np.all((pa.bs_v >> 2) <= 51) and np.all((pa.bs_h >> 2) <= 51)
            assert np.all((pa.bs_v & 3) <= 2) and np.all((pa.bs_h & 3) <= 2)
            assert all(abs(v) <= 12 for v in (pa.beta_offset, pa.tc_offset, pa.cb_qp_offset, pa.cr_qp_offset))
            assert pa.beta_offset % 2 == 0 and pa.tc_offset % 2 == 0
            for u in pa.pu:
                refs = [int(r) for r in u["ref"]]
                assert any(r >= 0 for r in refs) and all(r < a.n and r != pa.slot for r in refs)
            if pa.flags & (R.PIC_SAO_LUMA | R.PIC_SAO_CHROMA):
                s = pa.sao
                assert s["type"].max() <= 2 and s["band"].max() <= 31 and s["eo"].max() <= 3 and np.abs(s["off"]).max() <= 7
                e = s["type"] == 2
                assert np.all(s["off"][e][:, :2] >= 0) and np.all(s["off"][e][:, 2:] <= 0)
            # residuals: kinds only where legal, every coded block inside the pool, no two blocks sharing samples of it
            t, c_ = R._components(pa)
            kind, off = pa.tu["res"][t, c_], pa.tu["coef"][t, c_].astype(np.int64)
            n2 = 1 << (2 * pa.tu["log2"][t].astype(np.int64))
            l4 = pa.tu["log2"][t] == 2
            assert np.all(l4[kind == R.RES_SKIP])
            assert np.all((l4 & (pa.tu["plane"][t] == 0) & ((pa.tu["flags"][t] & 1) != 0))[kind == R.RES_DST])
            coded = kind != R.RES_NONE
            assert np.all(off[coded] + n2[coded] <= pa.n_coef)
            order = np.argsort(off[coded])
            assert np.all(off[coded][order][1:] >= (off[coded] + n2[coded])[order][:-1])
            for i in np.flatnonzero(kind == R.RES_DC):
                assert not pa.coef[off[i] + 1:off[i] + n2[i]].any()
            # what each family may touch
            own = {"mv": {"pu"}, "intra": {"tu"}, "resid": {"tu", "coef"}, "dbk": {"bs_v", "bs_h"}, "sao": {"sao"},
                   "flat": {"tu", "coef"}, "all": set(R.ARRAYS) - {"map"}}[family]
            for k in set(R.ARRAYS) - own:
                assert _equal(getattr(pa, k), getattr(p1, k)), k
            if family == "intra":
                for f in ("res", "coef"):
                    assert np.array_equal(pa.tu[f], p1.tu[f])
            if family in ("resid", "flat"):
                for f in ("mode", "strong"):
                    assert np.array_equal(pa.tu[f], p1.tu[f])
    assert differs_by_seed, "two seeds give the same records"


# a stream on which the family has something to change
SENSITIVE = {"mv": "cov_h265_hb_s1", "intra": "cov_h265_nosao_s1", "resid": "cov_h265_hiqp_s1", "dbk": "cov_h265_hb_s1",
             "sao": "cov_h265_nosao_s1", "flat": "cov_h265_pnodbk_s1", "all": "cov_h265_ldb_s1"}


@pytest.mark.parametrize("family", R.FAMILIES)
def test_mutation_changes_the_reconstruction(built, family):
    """A mutated list and its unmutated parent through two oracle back ends: the comparer reports a difference (a
    mutator that changes nothing the reconstruction reads would be a bug in the test), and names where."""
    name = SENSITIVE[family]
    parent, ref, _ = R.case(None, name, 0)
    if family == "flat":
        # (flat also changes the fill: compare under the same one, so that the records alone make the difference)
        parent = parent.clone()
        parent.fill = R.case(family, name, R.SEEDS[0])[0].fill
        ref, _ = R.oracle_replay(parent)
    rec, snaps, _ = R.case(family, name, R.SEEDS[0])
    assert R.first_difference(parent, ref, ref) is None
    msg = R.first_difference(rec, ref, snaps)
    assert msg is not None and msg.startswith("picture ") and "CTU (" in msg and "owner record" in msg, msg


def test_comparer_names_the_owner(built):
    """One byte changed by hand: the comparer names that picture, plane and position, and the record owning it."""
    rec, snaps, _ = R.case(None, "cov_h265_hb_s1", 0)
    other = [s.copy() for s in snaps]
    W, H = rec.width, rec.height
    x, y = 37, 22
    other[0][W * H + y * W + 2 * x + 1] ^= 0x40
    msg = R.first_difference(rec, snaps, other)
    p = rec[0]
    owner = int(p.map[(W // 4) * (H // 4) + (y >> 2) * (W // 8) + (x >> 2)])
    assert msg.splitlines()[0].startswith(f"picture 0 (slot {p.slot}") and f"Cr ({x}, {y})" in msg and "1 bytes differ" in msg
    assert f"owner record {owner}: x={int(p.tu[owner]['x'])}," in msg
    assert "vertical edge x=72" in msg and "horizontal edge y=40" in msg and "SAO record: type=" in msg


CASES = [(f, s) for f in R.FAMILIES for s in R.STREAMS]


@pytest.mark.parametrize("family", R.FAMILIES)
def test_domain_cap(built, family):
    """Outside the reference's defined domain (CLIP255C beyond [-256, 767], DC-only terms beyond the SWAR range: the
    oracle's violation count) the reference is undefined and the kernel need not match: such a case is skipped on
    the GPU, and at most one case in ten of a family may be.  The unmutated goldens stay at 0 (above)."""
    viol = {(s, seed): R.case(family, s, seed)[2] for s in R.STREAMS for seed in R.seeds(family)}
    skipped = [k for k, v in viol.items() if v]
    print(f"{family}: {len(viol)} cases, {len(skipped)} outside the reference's domain {skipped}")
    assert 10 * len(skipped) <= len(viol), viol


def test_seeds_cover_the_record_domain(built):
    """Summed over the committed (stream, seed) cases, counted from the mutated records: every deblocking QP 0..51
    with both bS values; every intra (mode, size, plane); every luma phase pair on a prediction block of each
    distinct shape present, and all 64 chroma phase pairs; every SAO edge class, SAO off and each band 28..31 on a
    CTU of the right column and of the bottom row."""
    cov = {}
    for family in ("mv", "intra", "dbk", "sao"):
        for s in R.STREAMS:
            for seed in R.seeds(family):
                R.coverage(R.case(family, s, seed)[0], cov)
    print({k: len(v) for k, v in cov.items()})
    assert cov["dbk_qp_bs"] >= {(q, b) for q in range(52) for b in (1, 2)}
    want = {(m, l2, 0) for m in range(35) for l2 in (2, 3, 4, 5)} | {(m, l2, 1) for m in range(35) for l2 in (2, 3, 4)}
    assert not want - cov["intra"], sorted(want - cov["intra"])
    assert {(12, 16), (16, 4), (64, 48)} <= cov["shapes"], cov["shapes"]  # (AMP shapes among them)
    missing = {(w, h, fx, fy) for (w, h) in cov["shapes"] for fx in range(4) for fy in range(4)} - cov["phase"]
    assert not missing, sorted(missing)
    assert len(cov["chroma_phase"]) == 64
    for where in ("right", "bottom"):
        assert {(where, e) for e in range(4)} <= cov["sao_edge"]
        assert {(where, b) for b in (28, 29, 30, 31)} <= cov["sao_band"]
        assert where in cov["sao_off"]


def test_resid_reaches_the_clips_and_the_global_coefficient_path(built):
    """What mutate_resid and mutate_flat are for, counted from their cases: CTUs whose pool range exceeds
    H265_CTU_COEF (stage_coef then reads global memory; the parser's contiguous pools never do, which the unmutated
    recordings show) beside CTUs that still stage into LDS, and a share of the reconstructed samples at each clip."""
    plain, cov = {}, {}
    for s in R.STREAMS:
        R.coverage(R.case(None, s, 0)[0], plain)
    assert "coef_global" not in plain and plain["coef_lds"]
    at0 = at255 = total = 0
    for s in R.STREAMS:
        for seed in R.SEEDS:
            rec, snaps, _ = R.case("resid", s, seed)
            R.coverage(rec, cov)
            for p, f in zip(rec, snaps):
                at0 += int((f == 0).sum())
                at255 += int((f == 255).sum())
                total += f.size
    print(f"resid: {len(cov['coef_global'])} CTU chunks read the pool globally, {len(cov['coef_lds'])} from LDS; "
          f"{100 * at0 / total:.1f} % of the samples at 0, {100 * at255 / total:.1f} % at 255")
    assert len(cov["coef_global"]) >= 100 and len(cov["coef_lds"]) >= 100
    assert at0 * 20 >= total and at255 * 20 >= total  # (one sample in 20 at each clip)
    for s in R.STREAMS:
        rec, snaps, _ = R.case("flat", s, R.SEEDS[0])
        i_pic = [f for p, f in zip(rec, snaps) if not p.n_pu][0]
        p = rec[0]
        inside = i_pic[:p.width * p.height].reshape(p.height, p.width)[:p.pic_h, :p.pic_w]
        assert inside.min() == inside.max() and int(inside.min()) in (0, 255)
