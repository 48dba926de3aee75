"""frisk_score_ranges_panel and python -m frisk_amd.regions --donors, as far as a machine without a GPU can tell: the header's
declarations against the binding, the nearest / margin rule on hand-made planes, the label collision, and the module end to end
on an engine whose panel answers from the numpy oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ranges_cases as R
import test_regions_cpu as TR

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAN = float("nan")


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_panel_symbols_and_constants_are_declared_as_bound():
    from frisk_amd import _ffi
    text = open(os.path.join(REPO, "include", "frisk_hip.h")).read()
    for name, value in (("FRISK_PANEL_MAX", _ffi.PANEL_MAX), ("FRISK_PANEL_TILE", _ffi.PANEL_TILE)):
        m = re.search(r"#define\s+%s\s+(\d+)\b" % name, text)
        assert m and int(m.group(1)) == value, name
    assert _ffi.PANEL_MAX % _ffi.PANEL_TILE == 0
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for decl in ("int frisk_panel_reset(frisk_ctx* ctx);", "int frisk_panel_push(frisk_ctx* ctx, int32_t* slot);",
                 "int32_t frisk_panel_size(const frisk_ctx* ctx);",
                 "int frisk_score_ranges_panel(frisk_ctx* ctx, const int32_t* seq_index, const int64_t* start, const int64_t* stop, "
                 "int64_t n, uint32_t flags, uint32_t* status, double* kld, double* gc, double* pi, double* si, double* cri, "
                 "int64_t* nn);"):
        assert decl in text, decl
    table = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    assert table["frisk_panel_reset"] == (C.c_int, [C.c_void_p])
    assert table["frisk_panel_push"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)])
    assert table["frisk_panel_size"] == (C.c_int32, [C.c_void_p])
    assert table["frisk_score_ranges_panel"] == table["frisk_score_ranges"]
    import __graft_entry__ as g
    g.build_hip()
    lib = _ffi.lib()
    assert lib.frisk_panel_reset(None) == _ffi.E_ARG and lib.frisk_panel_push(None, None) == _ffi.E_ARG
    assert lib.frisk_panel_size(None) == 0
    assert lib.frisk_score_ranges_panel(None, None, None, None, 0, 0, None, None, None, None, None, None, None) == _ffi.E_ARG
    from frisk_amd.engine import Engine
    from frisk_amd.hotpath import HotPath
    assert all(callable(getattr(Engine, m)) for m in ("panel_reset", "panel_push", "score_ranges_panel")) and callable(HotPath.scoreRegionsPanel)


# ------------------------------------------------------------------------------------------------------- nearest and margin
def test_nearest_and_margin_on_hand_made_planes():
    from frisk_amd import postprocess as pp
    from frisk_amd import regions
    from frisk_amd.engine import PanelResult
    K, ZW, NM = R.KEPT, R.KEPT | R.ZERO_WEIGHT, R.KEPT | R.NO_MAXMER
    # rows: a tie of the two best; all NaN; one finite cell; the int 0 beside NaN; an ordinary row; dropped by the N rule
    kld = np.array([[0.5, NAN, NAN, 0.0, 0.75, NAN],
                    [0.25, NAN, 1.5, NAN, 0.5, NAN],
                    [0.25, NAN, NAN, NAN, 2.0, NAN]])
    status = np.array([[K, ZW, ZW, NM, K, 0],
                       [K, ZW, K, ZW, K, 0],
                       [K, ZW, ZW, ZW, K, 0]], np.uint32)
    regs = [("c", 10 * r, 10 * r + 5, "r%d" % r) for r in range(6)]
    panel = PanelResult(status=status, kld=kld)
    labels = ["host.fa", "a.fa", "b.fa"]
    got = [l.rstrip("\n").split("\t") for l in regions.donor_rows(regs, panel, [0, 1, 2], labels, pp.py2_str)]
    assert regions.donor_columns(labels) == ["name", "start", "stop", "length", "id", "host.fa", "a.fa", "b.fa", "nearest", "margin"]
    assert got[0] == ["c", "1", "5", "5", "r0", "0.5", "0.25", "0.25", "a.fa", "0.0"]           # the first in column order wins
    assert got[1] == ["c", "11", "15", "5", "r1", "nan", "nan", "nan", ".", "."]
    assert got[2] == ["c", "21", "25", "5", "r2", "nan", "1.5", "nan", "a.fa", "."]
    assert got[3] == ["c", "31", "35", "5", "r3", "0", "nan", "nan", "host.fa", "."]
    assert got[4] == ["c", "41", "45", "5", "r4", "0.75", "0.5", "2.0", "a.fa", "0.25"]
    assert got[5] == ["c", "51", "55", "5", "r5", "nan", "nan", "nan", ".", "."]
    # the planes may be any slots of the panel, in column order
    swapped = [l.rstrip("\n").split("\t") for l in regions.donor_rows(regs, panel, [2, 0, 1], labels, pp.py2_str)]
    assert swapped[0][5:] == ["0.25", "0.5", "0.25", "host.fa", "0.0"] and swapped[4][5:] == ["2.0", "0.75", "0.5", "b.fa", "0.25"]
    assert regions.nearest_margin([]) == (None, None) and regions.nearest_margin([0, 0, NAN]) == (0, 0)


# ------------------------------------------------------------------------------------------ the module on an oracle engine
class _PanelEngine(TR._Engine):
    """test_regions_cpu's oracle engine with a panel: a slot is a copy of the finalised profile, a plane its score_ranges rows."""

    def __init__(self, kmin, kmax, device=0):
        super().__init__(kmin, kmax, device=device)
        self.panel = []

    def panel_reset(self):
        self.panel = []

    def panel_push(self):
        assert self.profile is not None
        sym, meta = self.profile
        self.panel.append((np.array(sym, dtype=np.int64), tuple(int(v) for v in meta)))
        return len(self.panel) - 1

    @property
    def panel_size(self):
        return len(self.panel)

    def score_ranges_panel(self, seq_index, start, stop, rip=False, big=False):
        from frisk_amd.engine import PanelResult
        assert self.panel
        mine, planes = self.profile, []
        for prof in self.panel:
            self.profile = prof
            planes.append(self.score_ranges(seq_index, start, stop, rip=rip))
        self.profile = mine
        cols = dict(planes[0].__dict__)
        cols.update(status=np.stack([p.status for p in planes]), kld=np.stack([p.kld for p in planes]))
        return PanelResult(**cols)


@pytest.fixture
def panel_regions(monkeypatch):
    from frisk_amd import hotpath, regions
    monkeypatch.setattr(hotpath, "Engine", _PanelEngine)
    real_init = hotpath.HotPath.__init__

    def init(self, kMin, kMax, device=0, cache_dir=None, use_cache=True):
        real_init(self, kMin, kMax, device=device, cache_dir=None, use_cache=use_cache)      # (no packed-sequence cache: no device)
    monkeypatch.setattr(hotpath.HotPath, "__init__", init)
    TR._Engine.adds = 0
    return regions


def _donors(tmp_path):
    rng = np.random.default_rng(11)
    paths = []
    for name, gc in (("d1.fa", 0.3), ("d2.fa", 0.7)):
        p = tmp_path / name
        p.write_text(">%s\n%s\n" % (name, R._bases(rng, 400, gc).decode()))
        paths.append(str(p))
    return paths


def _column(path, name):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    i = lines[0].split("\t").index(name)
    return [l.split("\t")[i] for l in lines[1:-1]]


def test_label_collision_ends_the_run(panel_regions, tmp_path, caplog):
    fa, bed, _ = TR._inputs(tmp_path)
    other = tmp_path / "elsewhere"
    other.mkdir()
    (other / "g.fa").write_text(">x\nACGTACGTAC\n")
    d1, d2 = _donors(tmp_path)
    out = tmp_path / "t"
    for donors in ([str(other / "g.fa")], [d1, d2, d1]):
        caplog.clear()
        assert panel_regions.main(["-H", fa, "-k", "4", "-t", str(out), "--bed", bed, "--donors"] + donors) == 1
        assert "--donors" in caplog.text
    assert not out.exists() and TR._Engine.adds == 0


def test_module_end_to_end_with_donors(panel_regions, tmp_path):
    fa, bed, _ = TR._inputs(tmp_path)
    d1, d2 = _donors(tmp_path)
    out, plain = tmp_path / "t", tmp_path / "plain"
    assert panel_regions.main(["-H", fa, "-k", "4", "-t", str(plain), "--bed", bed, "--RIP"]) == 0
    assert not (plain / "region_donor_scores.tsv").exists()                       # without --donors: today's path, one table
    TR._Engine.adds = 0
    argv = ["-H", fa, "-k", "4", "-t", str(out), "--bed", bed, "--RIP", "--donors", d1, d2]
    assert panel_regions.main(argv) == 0
    # -O: byte for byte the run without --donors
    assert (out / "region_scores.tsv").read_bytes() == (plain / "region_scores.tsv").read_bytes()
    # the caches of the main command line, one per genome, written by this run
    for name in ("g.fa", "d1.fa", "d2.fa"):
        assert (out / ("%s_kmers_1_4_genome.p" % name)).is_file(), name
    assert TR._Engine.adds == 3
    donor_file = out / "region_donor_scores.tsv"
    text = donor_file.read_text()
    assert text.split("\n")[0] == "name\tstart\tstop\tlength\tid\tg.fa\td1.fa\td2.fa\tnearest\tmargin"
    assert len(text.split("\n")) == 6 + 2
    for c in ("name", "start", "stop", "length", "id"):
        assert _column(donor_file, c) == _column(out / "region_scores.tsv", c), c
    # every cell = the windowKLD of a separate single-profile run (which reads the cache this run wrote)
    assert _column(donor_file, "g.fa") == _column(plain / "region_scores.tsv", "windowKLD")
    for d, name in ((d1, "d1.fa"), (d2, "d2.fa")):
        assert panel_regions.main(["-H", d, "-Q", fa, "-k", "4", "-t", str(out), "--bed", bed, "-O", name + ".tsv"]) == 0
        assert _column(donor_file, name) == _column(out / (name + ".tsv"), "windowKLD"), name
    assert TR._Engine.adds == 3
    # nearest / margin from the cells
    from frisk_amd import postprocess as pp
    cells = list(zip(*[_column(donor_file, n) for n in ("g.fa", "d1.fa", "d2.fa")]))
    labels = ["g.fa", "d1.fa", "d2.fa"]
    scored = 0
    for row, near, margin in zip(cells, _column(donor_file, "nearest"), _column(donor_file, "margin")):
        vals = [(float(v), i) for i, v in enumerate(row) if v != "nan"]
        if not vals:
            assert (near, margin) == (".", ".")
            continue
        assert near == labels[min(vals)[1]]
        if row == ("0", "0", "0"):
            assert margin == "0"                                                  # noMaxmer: the int 0 under every profile
        else:
            scored += 1
            assert float(margin) == pytest.approx(sorted(vals)[1][0] - sorted(vals)[0][0], abs=1e-11)
    assert scored == 1 and _column(out / "region_scores.tsv", "note").count("noMaxmer") == 3
    # the second run reads all three caches; --recalc (store_false) profiles all three again
    first = text
    assert panel_regions.main(argv + ["--donorOutfile", "again.tsv"]) == 0 and TR._Engine.adds == 3
    assert (out / "again.tsv").read_text() == first
    assert panel_regions.main(argv + ["--recalc"]) == 0 and TR._Engine.adds == 6
    assert donor_file.read_text() == first
