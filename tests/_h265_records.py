"""Record-level differential testing of the H.265 reconstruction back ends (helper; no tests in it).

The stream generator reaches a narrow slice of what the kernels accept through the record ABI (h265r_picture_t,
include/m2d_recon.h).  Here the records a real parse produced are captured (``record``), their *value* fields are
changed by seeded mutators (``mutate``), and the same pictures are submitted by hand to any back end (``replay``):
the CPU oracle and the gfx950 one must then give the same frames byte for byte (``first_difference``).

Geometry, record order, the 4 x 4 owner ``map`` and the availability counts always stay the parser's: the CTU
kernels' dependency waits depend only on those, so a mutated picture waits on exactly what an unmutated one does.
"""
import ctypes
import functools

import numpy as np

import m2dec_amd
from m2dec_amd import Backend265, Frame

RES_NONE, RES_DC, RES_FULL, RES_DST, RES_SKIP = 0, 1, 2, 3, 4
TU_PRED = 1
PIC_DEBLOCK, PIC_SAO_LUMA, PIC_SAO_CHROMA = 1, 2, 4


# ---------------------------------------------------------------- ctypes mirrors of include/m2d_recon.h
class TU(ctypes.Structure):
    """h265r_tu_t"""
    _fields_ = [("x", ctypes.c_uint16), ("y", ctypes.c_uint16), ("log2", ctypes.c_uint8), ("plane", ctypes.c_uint8),
                ("mode", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("avail_top", ctypes.c_int16),
                ("avail_left", ctypes.c_int16), ("res", ctypes.c_uint8 * 2), ("strong", ctypes.c_uint8),
                ("pad", ctypes.c_uint8), ("coef", ctypes.c_uint32 * 2)]


class PU(ctypes.Structure):
    """h265r_pu_t"""
    _fields_ = [("x", ctypes.c_uint16), ("y", ctypes.c_uint16), ("w", ctypes.c_uint8), ("h", ctypes.c_uint8),
                ("ref", ctypes.c_int8 * 2), ("mv", (ctypes.c_int16 * 2) * 2)]


class SAO(ctypes.Structure):
    """h265r_sao_t"""
    _fields_ = [("type", ctypes.c_uint8 * 3), ("band", ctypes.c_uint8 * 3), ("eo", ctypes.c_uint8 * 3),
                ("pad", ctypes.c_uint8 * 3), ("off", (ctypes.c_int8 * 4) * 3)]


class Picture(ctypes.Structure):
    """h265r_picture_t"""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("pic_w", ctypes.c_int32),
                ("pic_h", ctypes.c_int32), ("ctb_log2", ctypes.c_int32), ("slot", ctypes.c_int32),
                ("n_tu", ctypes.c_int32), ("n_coef", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("beta_offset", ctypes.c_int32), ("tc_offset", ctypes.c_int32), ("cb_qp_offset", ctypes.c_int32),
                ("cr_qp_offset", ctypes.c_int32), ("tu", ctypes.c_void_p), ("coef", ctypes.c_void_p),
                ("map", ctypes.c_void_p), ("bs_v", ctypes.c_void_p), ("bs_h", ctypes.c_void_p),
                ("sao", ctypes.c_void_p), ("n_pu", ctypes.c_int32), ("pu", ctypes.c_void_p)]


# the order of h265_oracle_layout (oracle/h265_oracle.c): per struct its size, then the offset of each field
LAYOUT = [(TU, [f for f, _ in TU._fields_]), (PU, [f for f, _ in PU._fields_]), (SAO, [f for f, _ in SAO._fields_]),
          (Picture, [f for f, _ in Picture._fields_]), (Backend265, [f for f, _ in Backend265._fields_])]


def python_layout():
    out = []
    for st, fields in LAYOUT:
        out.append(ctypes.sizeof(st))
        out += [getattr(st, f).offset for f in fields]
    return out


def c_layout():
    """The same numbers from the C compiler that built the oracle (offsetof / sizeof of include/m2d_recon.h)."""
    from _oracle import oracle_lib
    L = oracle_lib()
    L.h265_oracle_layout.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    L.h265_oracle_layout.restype = ctypes.c_int
    buf = (ctypes.c_int32 * 128)()
    n = L.h265_oracle_layout(buf, 128)
    assert 0 < n <= 128
    return list(buf[:n])


TU_DT, PU_DT, SAO_DT = np.dtype(TU), np.dtype(PU), np.dtype(SAO)
SCALARS = ("width", "height", "pic_w", "pic_h", "ctb_log2", "slot", "flags", "beta_offset", "tc_offset", "cb_qp_offset",
           "cr_qp_offset")
ARRAYS = ("tu", "coef", "map", "bs_v", "bs_h", "sao", "pu")


class Pic:
    """One picture's records in Python-owned arrays (a deep copy of an h265r_picture_t)."""

    def __init__(self, scalars, arrays):
        for k in SCALARS:
            setattr(self, k, int(scalars[k]))
        for k in ARRAYS:
            setattr(self, k, arrays[k])

    def copy(self):
        return Pic({k: getattr(self, k) for k in SCALARS}, {k: getattr(self, k).copy() for k in ARRAYS})

    @property
    def n_tu(self):
        return len(self.tu)

    @property
    def n_pu(self):
        return len(self.pu)

    @property
    def n_coef(self):
        return len(self.coef)

    @property
    def ctu_cols(self):
        return (self.pic_w + (1 << self.ctb_log2) - 1) >> self.ctb_log2

    @property
    def ctu_rows(self):
        return (self.pic_h + (1 << self.ctb_log2) - 1) >> self.ctb_log2

    def c_struct(self):
        """An h265r_picture_t over the arrays (which must stay alive and unchanged while it is used)."""
        W, H = self.width, self.height
        assert len(self.map) == (W // 4) * (H // 4) + (W // 8) * (H // 8)
        assert len(self.bs_v) == len(self.bs_h) == (H // 4) * (W // 8) and len(self.sao) == self.ctu_cols * self.ctu_rows
        p = Picture()
        for k in SCALARS:
            setattr(p, k, getattr(self, k))
        p.n_tu, p.n_coef, p.n_pu = self.n_tu, self.n_coef, self.n_pu
        for k in ARRAYS:
            a = getattr(self, k)
            assert a.flags["C_CONTIGUOUS"]
            setattr(p, k, a.ctypes.data)
        return p


class Recording(list):
    """The pictures of one stream in decoding order, with what a replay needs: the frame count and size the decoder
    gave set_frames, the output order (indices into the list) and an output frame's geometry (frame_md5's crop), and
    the replayer's initial fill (None: seeded pseudo-random bytes; else the byte every frame starts with)."""
    n = width = height = 0
    fill = None

    def __init__(self, *a):
        super().__init__(*a)
        self.output = []
        self.geom = None

    def clone(self):
        r = Recording(p.copy() for p in self)
        r.n, r.width, r.height, r.fill, r.output, r.geom = self.n, self.width, self.height, self.fill, list(self.output), self.geom
        return r


_SET_FRAMES = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Frame), ctypes.c_int, ctypes.c_int)
_SUBMIT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(Picture))
_SYNC = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int)
_DESTROY = ctypes.CFUNCTYPE(None, ctypes.c_void_p)


def _take(ptr, count, dtype):
    if not ptr or count <= 0:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer(ctypes.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()


# ---------------------------------------------------------------- the recording back end
def record(data):
    """The picture list of a stream: decode_h265 over an h265r_backend_t of ctypes callbacks (stage NULL) whose submit
    deep-copies every picture.  The parser never reads pixels, so the decode runs to its normal -2."""
    rec = Recording()
    luma, last, errs = [], {}, []

    def set_frames(_self, n, frames, w, h):
        try:
            assert not luma, "one geometry per stream"
            rec.n, rec.width, rec.height = n, w, h
            luma[:] = [frames[i].luma for i in range(n)]
            return 0
        except BaseException as e:  # noqa: BLE001 - re-raised after the C call returns
            errs.append(e)
            return -1

    def submit(_self, pp):
        try:
            p = pp.contents
            W, H = p.width, p.height
            ctb = 1 << p.ctb_log2
            nctu = ((p.pic_w + ctb - 1) // ctb) * ((p.pic_h + ctb - 1) // ctb)
            nbs = (H // 4) * (W // 8)
            arrays = {"tu": _take(p.tu, p.n_tu, TU_DT), "coef": _take(p.coef, p.n_coef, np.int16),
                      "map": _take(p.map, (W // 4) * (H // 4) + (W // 8) * (H // 8), np.int32),
                      "bs_v": _take(p.bs_v, nbs, np.uint8), "bs_h": _take(p.bs_h, nbs, np.uint8),
                      "sao": _take(p.sao, nctu, SAO_DT), "pu": _take(p.pu, p.n_pu, PU_DT)}
            last[p.slot] = len(rec)
            rec.append(Pic({k: getattr(p, k) for k in SCALARS}, arrays))
            return 0
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
            return -1

    cbs = [_SET_FRAMES(set_frames), _SUBMIT(submit), _SYNC(lambda _s, _slot: 0), _DESTROY(lambda _s: None)]
    be = Backend265()
    be.set_frames, be.submit, be.sync_frame, be.destroy = [ctypes.cast(c, ctypes.c_void_p).value for c in cbs]
    be.stage = None

    def on_frame(f):
        rec.output.append(last[luma.index(f.luma)])
        rec.geom = (f.width, f.height, tuple(f.crop))

    _, err = m2dec_amd.decode_h265(data, backend=be, on_frame=on_frame)
    if errs:
        raise errs[0]
    assert err == -2, err
    return rec


@functools.lru_cache(maxsize=None)
def recorded(name):
    """The recording of a golden stream (tests/golden/h265.json), made once; mutators copy it, nothing changes it."""
    from test_h265_cpu import h265_stream
    return record(h265_stream(name))


# ---------------------------------------------------------------- the replayer
def initial_frames(rec):
    """Every frame's starting bytes: the same for every back end, so that a reference slot read before any picture
    was written into it, and the bytes of a frame no block writes, are defined and equal on both sides."""
    size = rec.width * rec.height * 3 // 2
    if rec.fill is not None:
        return [np.full(size, rec.fill, dtype=np.uint8) for _ in range(rec.n)]
    return [np.random.default_rng(7000 + i).integers(0, 256, size, dtype=np.uint8) for i in range(rec.n)]


def replay(be, rec, prepare=None):
    """Submit the pictures to the h265r_backend_t ``be`` by hand (the unstaged path): set_frames over ``rec.n`` NV12
    frames of the whole width x height, then per picture submit, sync_frame(slot) and a snapshot of that frame.
    ``prepare`` runs after set_frames (the gfx950 back end: its device frames take the caller's bytes there).  Every
    status must be 0, the final sync_frame of every slot included (the CTU kernels report an exhausted wait there)."""
    W, H = rec.width, rec.height
    bufs = initial_frames(rec)
    frames = (Frame * rec.n)()
    for i, b in enumerate(bufs):
        frames[i].luma, frames[i].chroma = b.ctypes.data, b.ctypes.data + W * H
        frames[i].width, frames[i].height = W, H
    set_frames, submit, sync = _SET_FRAMES(be.set_frames), _SUBMIT(be.submit), _SYNC(be.sync_frame)
    assert set_frames(be.self, rec.n, frames, W, H) == 0
    if prepare is not None:
        prepare()
    snaps = []
    for k, p in enumerate(rec):
        cs = p.c_struct()
        assert submit(be.self, ctypes.byref(cs)) == 0, f"picture {k}: submit refused it"
        assert sync(be.self, p.slot) == 0, f"picture {k}: sync_frame({p.slot}) failed"
        snaps.append(bufs[p.slot].copy())
    for s in range(rec.n):
        assert sync(be.self, s) == 0, f"sync_frame({s}) failed after the replay"
    return snaps


def oracle_replay(rec):
    """(snapshots, domain violations) of a replay through the CPU oracle."""
    from _oracle import Oracle265Backend, h265_violations
    h265_violations(True)
    with Oracle265Backend() as o:
        snaps = replay(o.be, rec)
    return snaps, h265_violations(True)


def hip_replay(rec, device=0):
    """Snapshots of a replay through a fresh gfx950 back end (its environment switches are read at creation)."""
    with m2dec_amd.H265HipBackend(device) as h:
        return replay(h.be, rec, prepare=h.upload_frames)


def output_md5s(rec, snaps):
    """The snapshots hashed by frame_md5's rule, in output order."""
    out = []
    for k in rec.output:
        f = Frame()
        f.luma, f.chroma = snaps[k].ctypes.data, snaps[k].ctypes.data + rec.width * rec.height
        f.width, f.height = rec.geom[0], rec.geom[1]
        for i in range(4):
            f.crop[i] = rec.geom[2][i]
        out.append(m2dec_amd.frame_md5(f))
    return out


# ---------------------------------------------------------------- the comparer
def _fields(row):
    return ", ".join(f"{k}={row[k].tolist()}" for k in row.dtype.names if k != "pad")


def first_difference(rec, a, b):
    """None when the snapshot lists are equal; else a description of the first differing byte: picture, plane,
    (x, y), CTU, the record that owns its 4 x 4 unit (from ``map``) with its fields, the prediction block over it, the
    bS / QP bytes of the edges through its unit and the CTU's SAO record."""
    assert len(a) == len(b) == len(rec)
    for k, (fa, fb) in enumerate(zip(a, b)):
        if np.array_equal(fa, fb):
            continue
        p = rec[k]
        W, H = p.width, p.height
        i = int(np.flatnonzero(fa != fb)[0])
        n_diff = int(np.count_nonzero(fa != fb))
        if i < W * H:
            plane, y, x = "luma", i // W, i % W
            lx, ly = x, y
            unit = (y >> 2) * (W // 4) + (x >> 2)
        else:
            j = i - W * H
            y, x, comp = j // W, (j % W) >> 1, (j % W) & 1
            plane = "Cr" if comp else "Cb"
            lx, ly = 2 * x, 2 * y
            unit = (W // 4) * (H // 4) + (y >> 2) * (W // 8) + (x >> 2)
        msg = [f"picture {k} (slot {p.slot}, {'I' if not p.n_pu else 'P/B'}, {p.pic_w}x{p.pic_h} in {W}x{H}, CTB "
               f"{1 << p.ctb_log2}, flags {p.flags}): {plane} ({x}, {y}) is {int(fa[i])} vs {int(fb[i])}; {n_diff} bytes differ",
               f"  CTU ({lx >> p.ctb_log2}, {ly >> p.ctb_log2})"
               + ("" if lx < p.pic_w and ly < p.pic_h else " - outside the picture")]
        owner = int(p.map[unit])
        if 0 <= owner < p.n_tu:
            msg.append(f"  owner record {owner}: {_fields(p.tu[owner])}")
        else:
            msg.append(f"  owner record: none (map {owner})")
        for n, u in enumerate(p.pu):
            if u["x"] <= lx < u["x"] + u["w"] and u["y"] <= ly < u["y"] + u["h"]:
                msg.append(f"  prediction block {n}: {_fields(u)}")
        bv = p.bs_v[(ly >> 2) * (W // 8) + (lx >> 3)]
        bh = p.bs_h[(ly >> 3) * (W // 4) + (lx >> 2)]
        msg.append(f"  vertical edge x={lx & ~7}: bS {bv & 3} QP {bv >> 2}; horizontal edge y={ly & ~7}: bS {bh & 3} QP {bh >> 2}; "
                   f"beta/tc offsets {p.beta_offset}/{p.tc_offset}, cb/cr {p.cb_qp_offset}/{p.cr_qp_offset}")
        if lx < p.pic_w and ly < p.pic_h:
            msg.append(f"  SAO record: {_fields(p.sao[(ly >> p.ctb_log2) * p.ctu_cols + (lx >> p.ctb_log2)])}")
        return "\n".join(msg)
    return None


# ---------------------------------------------------------------- mutators
FAMILIES = ("mv", "intra", "resid", "dbk", "sao", "flat", "all")


def _rng(seed, family):
    return np.random.default_rng([int(seed), FAMILIES.index(family)])


def mutate_mv(rec, seed):
    """Every prediction block's references and vectors; position and size never (overlapping blocks would race).

    Each block becomes uni-L0, uni-L1 or bi-predicted whatever it was, its references drawn among the slots below
    ``rec.n`` that are not the picture's own (both lists may name the same slot; a slot no picture was written into
    yet holds the replayer's fill).  Vectors: the luma phase pairs are dealt in turn per block shape (so every shape
    meets all 16), on an integer part that is near the block, or puts the window (the block plus the filter taps)
    around the left / right / top / bottom picture edge, from wholly outside to partly inside, each axis on its own
    (so corners too); one vector in 16 takes int16 extremes (+-32767, -32768) in one or both components.  A shape with
    fewer than 16 blocks in the stream (the large AMP ones: one 64 x 48 block) is always bi-predicted, without
    extremes, and seed s deals it the turns from 2 (s - 1) count on: 8 seeds give a single block all 16 pairs.  Both
    sides clamp every position into the picture and compute in 32 / 64-bit integers, so every int16 value is safe."""
    out, rng = rec.clone(), _rng(seed, "mv")
    count = {}
    for p in out:
        for u in p.pu:
            count[(int(u["w"]), int(u["h"]))] = count.get((int(u["w"]), int(u["h"])), 0) + 1
    turn = {sh: 2 * (int(seed) - 1) * c if c < 16 else int(seed) * 5 for sh, c in count.items()}
    for p in out:
        slots = [s for s in range(out.n) if s != p.slot]
        for u in p.pu:
            w, h, x, y = int(u["w"]), int(u["h"]), int(u["x"]), int(u["y"])
            rare = count[(w, h)] < 16
            kind = 2 if rare else rng.choice(3, p=[0.3, 0.2, 0.5])
            for l in range(2):
                if kind != 2 and l != kind:
                    u["ref"][l] = -1
                    u["mv"][l] = 0
                    continue
                u["ref"][l] = slots[rng.integers(len(slots))]
                t = turn[(w, h)]
                turn[(w, h)] = t + 1
                frac = (t & 3, (t >> 2) & 3)
                for ax, (pos, size, lim) in enumerate(((x, w, p.pic_w), (y, h, p.pic_h))):
                    r = rng.random()
                    if r < 0.5:
                        ipos = pos + int(rng.integers(-12, 13))
                    elif r < 0.75:
                        ipos = -size + int(rng.integers(-9, 10))
                    else:
                        ipos = lim - int(rng.choice([0, size])) + int(rng.integers(-9, 10))
                    u["mv"][l][ax] = 4 * (ipos - pos) + frac[ax]
                if not rare and rng.random() < 1 / 16:
                    ext = (32767, -32768, -32767)
                    which = rng.integers(1, 4)
                    for ax in range(2):
                        if (which >> ax) & 1:
                            u["mv"][l][ax] = ext[rng.integers(3)]
    return out


def mutate_intra(rec, seed):
    """``mode`` in 0..34 for every H265R_TU_PRED record of both planes, ``strong`` toggled on luma.  Per (plane, size)
    the modes are dealt in turn over a random half of the blocks (so that every mode meets every size) and uniformly
    at random over the rest.  Both sides index their 35-entry angle tables with the mode and nothing else."""
    out, rng = rec.clone(), _rng(seed, "intra")
    turn = {}
    for p in out:
        tu = p.tu
        pred = (tu["flags"] & TU_PRED) != 0
        for pl in (0, 1):
            for l2 in (2, 3, 4, 5):
                idx = np.flatnonzero(pred & (tu["plane"] == pl) & (tu["log2"] == l2))
                if not len(idx):
                    continue
                modes = rng.integers(0, 35, len(idx))
                dealt = np.flatnonzero(rng.random(len(idx)) < 0.5) if len(idx) > 8 else np.arange(len(idx))
                t = turn.get((pl, l2), int(seed) * 13)
                modes[dealt] = (t + np.arange(len(dealt))) % 35
                turn[(pl, l2)] = t + len(dealt)
                tu["mode"][idx] = modes
        luma = np.flatnonzero(pred & (tu["plane"] == 0))
        tu["strong"][luma] ^= rng.integers(0, 2, len(luma)).astype(np.uint8)
    return out


def _components(p):
    """(record index, component) of every residual a picture's records carry: luma [0]; chroma Cb [0], Cr [1]."""
    t = np.concatenate([np.arange(p.n_tu), np.flatnonzero(p.tu["plane"] == 1)])
    c = np.concatenate([np.zeros(p.n_tu, dtype=np.int64), np.ones(len(t) - p.n_tu, dtype=np.int64)])
    return t, c


def _place(p, t, c, kinds):
    """Give component c of record t the residual kind kinds[i] (RES_NONE: left as it is): a coded one keeps its pool
    offset, a new one is appended at the end of the pool.  Returns (the new zeroed pool, offsets, sizes)."""
    tu = p.tu
    n2 = 1 << (2 * tu["log2"][t].astype(np.int64))
    cur = tu["res"][t, c]
    off = tu["coef"][t, c].astype(np.int64)
    new = (cur == RES_NONE) & (kinds != RES_NONE)
    off[new] = p.n_coef + np.cumsum(n2[new]) - n2[new]
    set_ = kinds != RES_NONE
    tu["res"][t[set_], c[set_]] = kinds[set_]
    tu["coef"][t[set_], c[set_]] = off[set_]
    return np.zeros(p.n_coef + int(n2[new].sum()), dtype=np.int16), off, n2


def mutate_resid(rec, seed, only=None):
    """Coefficient values of every coded block, and its residual kind where a switch is legal: DC-only <-> full on any
    size (a DC-only block keeps coef[0] alone), DST only on intra luma 4 x 4, transform skip only on 4 x 4; four in
    ten uncoded blocks become coded, their coefficients appended at the end of the pool (n_coef grows), which takes a
    CTU's pool range past H265_CTU_COEF: stage_coef's global-read path.

    Amplitudes are bounded so that no case leaves the reference's defined domain (the oracle's violation count stays
    0), yet most blocks saturate samples at 0 and 255.  A residual r added to a prediction in 0..255 must keep the
    sum in CLIP255C's [-256, 767], so |r| <= 256:
      full: 1..6 coefficients, low frequencies preferred, sum |c| <= 15000: |r| <= sum |c| 90 90 / 2^19 + 1 < 234
            (DST: 84 84 / 2^19, < 204);
      DC-only: coef[0] in [-32704, 32703], half of them in the outer 8 %: |(c + 64) >> 7| <= 255, the byte range
            of the reference's SWAR add;
      transform skip: |c| <= 8000: |(c + 16) >> 5| <= 250."""
    out, rng = rec.clone(), _rng(seed, "resid")
    for k, p in enumerate(out):
        if only is not None and k not in only:
            continue
        t, c = _components(p)
        tu = p.tu
        l2, cur = tu["log2"][t], tu["res"][t, c]
        intra_luma4 = (l2 == 2) & (tu["plane"][t] == 0) & ((tu["flags"][t] & TU_PRED) != 0)
        kinds = rng.choice([RES_DC, RES_FULL, RES_DST, RES_SKIP], p=[0.3, 0.5, 0.1, 0.1], size=len(t))
        kinds[(kinds == RES_DST) & ~intra_luma4] = RES_FULL
        kinds[(kinds == RES_SKIP) & (l2 != 2)] = RES_FULL
        kinds[(cur == RES_NONE) & (rng.random(len(t)) >= 0.4)] = RES_NONE
        pool, off, n2 = _place(p, t, c, kinds)
        n = 1 << l2.astype(np.int64)
        # DC-only
        dc = np.flatnonzero(kinds == RES_DC)
        mag = np.where(rng.random(len(dc)) < 0.5, rng.integers(30000, 32704, len(dc)), rng.integers(0, 32704, len(dc)))
        pool[off[dc]] = np.where(rng.random(len(dc)) < 0.5, mag, -mag - 1)
        # transform skip: every sample of the 4 x 4
        sk = np.flatnonzero(kinds == RES_SKIP)
        pos = (off[sk][:, None] + np.arange(16)[None, :]).ravel()
        pool[pos] = rng.integers(-8000, 8001, len(pos))
        # full / DST: up to 6 coefficients sharing a budget (a later one on the same position replaces the earlier)
        fu = np.flatnonzero((kinds == RES_FULL) | (kinds == RES_DST))
        budget = 15000 * rng.choice([0.03, 0.2, 0.6, 1.0], p=[0.15, 0.2, 0.3, 0.35], size=len(fu))
        share = rng.random((len(fu), 6)) * (np.arange(6)[None, :] < rng.integers(1, 7, len(fu))[:, None])
        share = share / share.sum(axis=1, keepdims=True)
        val = np.floor(budget[:, None] * share).astype(np.int64) * rng.choice([-1, 1], size=share.shape)
        fy = np.minimum(rng.geometric(0.35, share.shape) - 1, n[fu][:, None] - 1)
        fx = np.minimum(rng.geometric(0.35, share.shape) - 1, n[fu][:, None] - 1)
        for j in range(6):  # (in turn: a duplicate position keeps one value, never a sum past the budget)
            pool[off[fu] + fy[:, j] * n[fu] + fx[:, j]] = val[:, j]
        p.coef = pool
    return out


def mutate_dbk(rec, seed):
    """Every nonzero bs_v / bs_h byte gets a QP in 0..51 and a bS in {1, 2}, or (one in ten) is cleared; bytes the
    parser left 0 stay 0 (an edge it never marked may have no samples on its far side).  Per picture beta_offset and
    tc_offset are even in -12..12, cb / cr_qp_offset in -12..12, and the deblocking flag is set.  Both sides clip
    qp + offset into their tables (0..51 luma, 0..53 chroma after qpc_deb, which takes qp + offset in -12..63)."""
    out, rng = rec.clone(), _rng(seed, "dbk")
    for p in out:
        for arr in (p.bs_v, p.bs_h):
            new = ((rng.integers(0, 52, len(arr)) << 2) | rng.integers(1, 3, len(arr))).astype(np.uint8)
            new[rng.random(len(arr)) < 0.1] = 0
            nz = arr != 0
            arr[nz] = new[nz]
        p.beta_offset, p.tc_offset = (2 * int(v) for v in rng.integers(-6, 7, 2))
        p.cb_qp_offset, p.cr_qp_offset = (int(v) for v in rng.integers(-12, 13, 2))
        p.flags |= PIC_DEBLOCK
    return out


def mutate_sao(rec, seed):
    """Per CTU and component: type 0 / 1 / 2, band 0..31 (half of them in 28..31, the no-wrap quirk), edge class 0..3
    (Cr takes Cb's, as the record says), band offsets of any sign up to 7, edge offsets >= 0 for categories 1, 2 and
    <= 0 for 3, 4; the picture's luma and chroma SAO flags are set.  Neither side indexes a table with these."""
    out, rng = rec.clone(), _rng(seed, "sao")
    for p in out:
        s, n = p.sao, len(p.sao)
        s["type"] = rng.choice(3, p=[0.2, 0.4, 0.4], size=(n, 3))
        s["band"] = np.where(rng.random((n, 3)) < 0.5, rng.integers(28, 32, (n, 3)), rng.integers(0, 32, (n, 3)))
        eo = rng.integers(0, 4, (n, 3))
        eo[:, 2] = eo[:, 1]
        s["eo"] = eo
        s["pad"] = 0
        band = rng.integers(-7, 8, (n, 3, 4))
        edge = rng.integers(0, 8, (n, 3, 4)) * np.array([1, 1, -1, -1])
        s["off"] = np.where((s["type"] == 2)[:, :, None], edge, band)
        p.flags |= PIC_SAO_LUMA | PIC_SAO_CHROMA
    return out


def mutate_flat(rec, seed):
    """Saturated reference pictures: the replayer's initial fill becomes all 0 or all 255, and every block of every
    I picture gets a DC-only residual of -255 or +255 (coef[0] = -32704 / 32703, inside the SWAR byte range), which
    saturates the whole picture whatever its prediction; the record structure is untouched.  Motion compensation,
    deblocking and SAO of the pictures that follow then run on samples at the clips.  Those pictures' coefficients
    are halved: their residuals were in CLIP255C's domain on top of the stream's own mid-grey predictions
    (r in [-511, 767]), and must now be so on top of 0 and 255 (r in [-256, 512])."""
    out = rec.clone()
    out.fill = 255 if seed & 1 else 0
    i_pics = 0
    for p in out:
        if p.n_pu:
            p.coef >>= 1
            continue
        up = ((seed >> 1) + i_pics) & 1
        i_pics += 1
        t, c = _components(p)
        pool, off, _ = _place(p, t, c, np.full(len(t), RES_DC, dtype=np.uint8))
        pool[off] = 32703 if up else -32704
        p.coef = pool
    return out


def mutate_all(rec, seed):
    """Every family at once.  Odd seeds keep flat's saturated I pictures (resid then changes the other pictures
    only); even seeds let resid rewrite them too, under flat's fill."""
    out = mutate_flat(rec, seed)
    keep = [k for k, p in enumerate(out) if p.n_pu] if seed & 1 else None
    out = mutate_resid(out, seed, only=keep)
    for f in (mutate_mv, mutate_intra, mutate_dbk, mutate_sao):
        out = f(out, seed)
    return out


MUTATORS = {"mv": mutate_mv, "intra": mutate_intra, "resid": mutate_resid, "dbk": mutate_dbk, "sao": mutate_sao,
            "flat": mutate_flat, "all": mutate_all}

# the smallest geometry per CTB size and slice type: 160 x 96 CTB 16 intra; CTB 64 intra with 32 x 32 blocks;
# 168 x 104 CTB 16 P (deblocking off in the stream); B CTB 16; B CTB 64 with AMP, size no CTB multiple
STREAMS = ("cov_h265_hiqp_s1", "cov_h265_nosao_s1", "cov_h265_pnodbk_s1", "cov_h265_hb_s1", "cov_h265_ldb_s1")
SEEDS = (1, 2, 3)
MV_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)  # (mutate_mv: a shape with a single block needs 8 seeds for the 16 phase pairs)


def seeds(family):
    return MV_SEEDS if family == "mv" else SEEDS


VARIANT_STREAMS = ("cov_h265_nosao_s1", "cov_h265_ldb_s1")


@functools.lru_cache(maxsize=None)
def case(family, stream, seed):
    """(the mutated recording, the oracle's snapshots of it, its domain violations), computed once and shared."""
    rec = MUTATORS[family](recorded(stream), seed) if family else recorded(stream)
    snaps, viol = oracle_replay(rec)
    return rec, snaps, viol


# ---------------------------------------------------------------- coverage of the mutated records
def coverage(rec, cov):
    """Add what the recording's records reach to ``cov`` (a dict of sets)."""
    for p in rec:
        if p.flags & PIC_DEBLOCK:
            for arr in (p.bs_v, p.bs_h):
                nz = arr[arr != 0]
                cov.setdefault("dbk_qp_bs", set()).update(zip((nz >> 2).tolist(), (nz & 3).tolist()))
        tu = p.tu[(p.tu["flags"] & TU_PRED) != 0]
        cov.setdefault("intra", set()).update(zip(tu["mode"].tolist(), tu["log2"].tolist(), tu["plane"].tolist()))
        for u in p.pu:
            for l in range(2):
                if u["ref"][l] >= 0:
                    mv = u["mv"][l]
                    cov.setdefault("phase", set()).add((int(u["w"]), int(u["h"]), int(mv[0]) & 3, int(mv[1]) & 3))
                    cov.setdefault("chroma_phase", set()).add((int(mv[0]) & 7, int(mv[1]) & 7))
            cov.setdefault("shapes", set()).add((int(u["w"]), int(u["h"])))
        # the pool range of each CTU's records (per chunk of H265_CTU_RECS = 256, as the CTU kernels stage them):
        # past H265_CTU_COEF = 6144 coefficients stage_coef reads the pool from global memory instead of LDS
        t, c = _components(p)
        coded = p.tu["res"][t, c] != RES_NONE
        t, off = t[coded], p.tu["coef"][t, c][coded].astype(np.int64)
        sub = p.tu["plane"][t].astype(np.int64)
        ctu = ((p.tu["y"][t].astype(np.int64) << sub) >> p.ctb_log2) * p.ctu_cols + ((p.tu["x"][t].astype(np.int64) << sub) >> p.ctb_log2)
        all_sub = p.tu["plane"].astype(np.int64)
        all_ctu = ((p.tu["y"].astype(np.int64) << all_sub) >> p.ctb_log2) * p.ctu_cols + ((p.tu["x"].astype(np.int64) << all_sub) >> p.ctb_log2)
        first = np.searchsorted(all_ctu, np.arange(p.ctu_cols * p.ctu_rows))  # (CTUs in raster order: check_picture)
        chunk = ctu * 4096 + (t - first[ctu]) // 256
        hi = off + (1 << (2 * p.tu["log2"][t].astype(np.int64)))
        for ch in np.unique(chunk):
            m = chunk == ch
            cov.setdefault("coef_global" if hi[m].max() - off[m].min() > 6144 else "coef_lds", set()).add((id(p), int(ch)))
        if p.flags & (PIC_SAO_LUMA | PIC_SAO_CHROMA):
            cols, rows = p.ctu_cols, p.ctu_rows
            for i, s in enumerate(p.sao):
                where = [w for w, on in (("right", i % cols == cols - 1), ("bottom", i // cols == rows - 1)) if on]
                for ci in range(3):
                    if not p.flags & (PIC_SAO_CHROMA if ci else PIC_SAO_LUMA):
                        continue
                    ty = int(s["type"][ci])
                    for w in where:
                        if ty == 2:
                            cov.setdefault("sao_edge", set()).add((w, int(s["eo"][ci])))
                        elif ty == 1:
                            cov.setdefault("sao_band", set()).add((w, int(s["band"][ci])))
                        else:
                            cov.setdefault("sao_off", set()).add(w)
    return cov
