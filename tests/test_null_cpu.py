"""The null model of python -m frisk_amd.regions --null, as far as a machine without a GPU can tell: the C ABI's symbol, the numpy
generator (frisk_amd/nullmodel.py, the specification of csrc/null_kernels.h) on tables that can be checked by hand and against a
scalar restatement in Python integers, the host draws, the statistics, and the module end to end on an oracle engine."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kld_oracle_hp as H
from golden_util import INPUTS
from oracle import frisk_oracle_np as N
from test_regions_cpu import _Engine

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
U64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# -------------------------------------------------------------------------------------------------------------------- ABI
def test_null_symbol_is_declared_listed_and_exported():
    import __graft_entry__ as g
    g.build_hip()
    from frisk_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "frisk_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+frisk_seq_null\s*\(\s*frisk_ctx\s*\*\s*ctx\s*,\s*const\s+int64_t\s*\*\s*lens\s*,\s*int32_t\s+n_seq\s*,"
                     r"\s*uint64_t\s+seed\s*,\s*int32_t\s+order\s*\)", text)
    table = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    assert table["frisk_seq_null"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_uint64, C.c_int32])
    lib = _ffi.lib()
    assert lib.frisk_seq_null(None, None, 0, 0, 0) == _ffi.E_ARG
    assert lib.frisk_last_kernel_ms(None, 6) == -1.0
    from frisk_amd.engine import Engine
    from frisk_amd.hotpath import HotPath
    assert callable(Engine.null_batch) and callable(HotPath.nullScores)
    assert os.path.isfile(os.path.join(REPO, "frisk_amd", "csrc", "null_kernels.h"))


# ------------------------------------------------------------------------------------------------------------ the generator
def _sym(kmin, kmax, order, rows):
    """A profile's flat symmetric counts, zero but for the table of order `order` + 1 = `rows` (4^order rows of four)."""
    from frisk_amd.engine import profile_len, table_offset
    sym = np.zeros(profile_len(kmin, kmax), dtype=np.int64)
    flat = [int(v) for row in rows for v in row]
    assert len(flat) == 4 ** (order + 1)
    off = table_offset(kmin, order + 1)
    sym[off:off + len(flat)] = flat
    return sym


def _scalar(rows, order, seed, seq, length):
    """The definition, one base at a time in Python integers: (x * T) >> 64 is the big-integer product."""
    from frisk_amd.nullmodel import mix_int
    out = bytearray()
    for blk in range((length + 4095) // 4096):
        state = mix_int((seed & U64) ^ mix_int(((seq << 40) ^ blk ^ (12 << 56)) & U64))
        ctx = 0
        for step in range(64 + min(4096, length - 4096 * blk)):
            state = (state + GOLDEN) & U64
            x = mix_int(state)
            cum = [sum(int(v) for v in rows[ctx][:b + 1]) for b in range(4)]
            if cum[3] == 0:
                b = x >> 62
            else:
                u = (x * cum[3]) >> 64
                b = (u >= cum[0]) + (u >= cum[1]) + (u >= cum[2])
            ctx = ((ctx << 2) | b) & (4 ** order - 1)
            if step >= 64:
                out.append(b"ATGC"[b])
    return bytes(out)


def test_mix_and_mulhi_agree_with_python_integers():
    from frisk_amd import nullmodel as M
    from frisk_amd.synth import _mix
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 63, 200, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 200, dtype=np.uint64)
    t = np.concatenate([rng.integers(0, 1 << 63, 196, dtype=np.uint64), np.array([0, 1, U64, 1 << 32], dtype=np.uint64)])
    assert [int(v) for v in M.mulhi64(x, t)] == [(int(a) * int(b)) >> 64 for a, b in zip(x, t)]
    assert [int(v) for v in _mix(x)] == [M.mix_int(int(a)) for a in x]


def test_order_0_with_a_single_count_gives_all_a():
    from frisk_amd import nullmodel as M
    assert M.generate(_sym(1, 3, 0, [[1, 0, 0, 0]]), 1, 0, 5, 0, 5000) == b"A" * 5000
    assert M.generate(_sym(1, 3, 0, [[0, 0, 0, 9]]), 1, 0, 5, 2, 70) == b"C" * 70


def test_order_1_cycle_at_the_phase_the_burn_in_leaves():
    """A -> T -> G -> C -> A from context 0 (= A): step s gives digit (s + 1) % 4, position t is step 64 + t: T first, in every
    block (4096 and 64 are multiples of 4: a restart shows as nothing)."""
    from frisk_amd import nullmodel as M
    sym = _sym(1, 2, 1, [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0]])
    for seed, seq in ((0, 0), (77, 3)):
        assert M.generate(sym, 1, 1, seed, seq, 8195) == (b"TGCA" * 2049)[:8195]
    sym3 = _sym(2, 3, 1, [[0, 7, 0, 0], [0, 0, 7, 0], [0, 0, 0, 7], [7, 0, 0, 0]])     # the same table behind another kmin
    assert M.generate(sym3, 2, 1, 1, 0, 10) == b"TGCATGCATG"


def test_empty_context_takes_the_top_two_bits():
    """Context A has no counts (b = x >> 62), every other context goes back to A."""
    from frisk_amd import nullmodel as M
    rows = [[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]]
    got = M.generate(_sym(1, 2, 1, rows), 1, 1, 9, 1, 4200)
    assert got == _scalar(rows, 1, 9, 1, 4200)
    assert set(got) == set(b"ATGC")
    assert all(got[i + 1:i + 2] == b"A" for i in range(len(got) - 1) if got[i:i + 1] != b"A" and (i + 1) % 4096)


def test_counts_above_2_32_agree_with_the_big_integer_product():
    from frisk_amd import nullmodel as M
    rng = np.random.default_rng(11)
    rows = [[int(v) for v in rng.integers(1, 1 << 61, 4)] for _ in range(16)]
    rows[5] = [(1 << 62) - 1, 1, 0, (1 << 33) + 5]
    assert max(sum(r) for r in rows) < 1 << 63 and max(sum(r) for r in rows) > 1 << 33
    for seq, n in ((0, 300), (2, 4100)):
        assert M.generate(_sym(1, 3, 2, rows), 1, 2, 123456789, seq, n) == _scalar(rows, 2, 123456789, seq, n)
    # ... and a table of ordinary counts of a real profile, order 3 behind kmin = 2
    seqs = H.read_fasta(os.path.join(INPUTS, "markov_islands.fa"))
    sym, _ = N.genome_profile(seqs, 2, 5)
    from frisk_amd.engine import table_offset
    rows = sym[table_offset(2, 4):table_offset(2, 5)].reshape(-1, 4).tolist()
    assert M.generate(sym, 2, 3, 2 ** 64 - 3, 7, 4200) == _scalar(rows, 3, 2 ** 64 - 3, 7, 4200)


def test_prefix_property_and_the_batch_form():
    from frisk_amd import nullmodel as M
    seqs = H.read_fasta(os.path.join(INPUTS, "markov_islands.fa"))
    sym, _ = N.genome_profile(seqs, 1, 6)
    long = M.generate(sym, 1, 5, 4, 2, 9000)
    for n in (1, 63, 64, 65, 4095, 4096, 4097, 8193):
        assert M.generate(sym, 1, 5, 4, 2, n) == long[:n]
    batch = M.generate_batch(sym, 1, 5, 4, [10, 0, 9000, 4096])
    assert batch[2] == long and batch[1] == b"" and [len(b) for b in batch] == [10, 0, 9000, 4096]
    assert batch[0] == M.generate(sym, 1, 5, 4, 0, 10) and batch[3] == M.generate(sym, 1, 5, 4, 3, 4096)
    assert batch[0] != long[:10] or batch[3] != long[:4096]             # the sequence index enters
    assert M.generate(sym, 1, 5, 5, 2, 9000) != long                     # ... and the seed
    assert M.generate(sym, 1, 5, 4, 2, 0) == b"" and M.generate_batch(sym, 1, 5, 4, []) == []


def test_transition_frequencies_follow_the_profile():
    """200 000 bases at order 3 from the profile of markov_islands.fa: every (context, base) cell with an expected count of 100 or
    more within 5 binomial standard deviations (a fair generator fails with probability < 2e-4 over the 256 cells).  A position's
    context is its three predecessors in the output from the fourth base of a block on."""
    from frisk_amd import nullmodel as M
    from frisk_amd.engine import table_offset
    seqs = H.read_fasta(os.path.join(INPUTS, "markov_islands.fa"))
    sym, _ = N.genome_profile(seqs, 1, 8)
    rows = sym[table_offset(1, 4):table_offset(1, 5)].reshape(64, 4).astype(np.float64)
    digit = np.full(256, -1)
    for i, ch in enumerate(b"ATGC"):
        digit[ch] = i
    d = digit[np.frombuffer(M.generate(sym, 1, 3, 20240611, 0, 200000), dtype=np.uint8)]
    assert d.min() == 0 and d.max() == 3
    t = np.arange(3, d.size)
    t = t[t % 4096 >= 3]
    ctx = d[t - 3] * 16 + d[t - 2] * 4 + d[t - 1]
    seen = np.bincount(ctx * 4 + d[t], minlength=256).reshape(64, 4).astype(np.float64)
    n_ctx = seen.sum(axis=1, keepdims=True)
    p = rows / rows.sum(axis=1, keepdims=True)
    expect = n_ctx * p
    sd = np.sqrt(n_ctx * p * (1 - p))
    big = expect >= 100
    assert big.sum() >= 200
    worst = float((np.abs(seen - expect)[big] / sd[big]).max())
    print("transition cells checked %d, worst deviation %.2f sd" % (int(big.sum()), worst))
    assert worst <= 5.0


# ----------------------------------------------------------------------------------------------------------- the host draws
def test_host_draws_stay_inside_and_reach_both_ends():
    from frisk_amd import nullmodel as M
    lens = [5, 2, 3]
    got = M.host_draws(lens, 3, 400, 1)
    assert len(got) == 400 and set(got) == {(0, 0), (0, 1), (0, 2), (2, 0)}              # the first and the last start included
    for L in (1, 2, 3, 4, 5):
        for s, a in M.host_draws(lens, L, 100, 8):
            assert 0 <= a and a + L <= lens[s]
    assert M.host_draws(lens, 6, 10, 1) == [] and M.host_draws([], 1, 10, 1) == []
    # the definition in Python integers
    total = 3 + 1
    for j, (s, a) in enumerate(got[:50]):
        idx = (M.mix_int(1 ^ M.mix_int((3 << 24) ^ j ^ (13 << 56))) * total) >> 64
        assert (s, a) == ((0, idx) if idx < 3 else (2, idx - 3))
    assert M.host_draws(lens, 3, 400, 2) != got and M.host_draws(lens, 3, 20, 1) == got[:20]
    big = M.host_draws([1 << 40, 1 << 41], 1 << 39, 50, 5)                               # totals past 2^32
    assert all(0 <= a <= [1 << 40, 1 << 41][s] - (1 << 39) for s, a in big) and {s for s, _ in big} == {0, 1}


# ----------------------------------------------------------------------------------------------------------- the statistics
def test_statistics_on_hand_made_arrays():
    from frisk_amd import nullmodel as M
    n, mean, sd, excess, z, p = M.stats(3.0, [1.0, 2.0, 3.0, 4.0])
    assert (n, mean, excess) == (4, 2.5, 0.5) and sd == math.sqrt(5.0 / 3.0) and z == 0.5 / sd
    assert p == (1 + 2) / 5.0                                                           # 3.0 ties with one draw: it counts
    assert M.stats(5.0, [1.0, 2.0])[5] == 1 / 3.0 and M.stats(0.5, [1.0, 2.0])[5] == 1.0
    assert M.stats(1.0, []) == (None,) * 6
    assert M.stats(1.5, [1.0]) == (1, 1.0, None, 0.5, None, 0.5)
    assert M.stats(2.0, [2.0, 2.0, 2.0]) == (3, 2.0, 0.0, 0.0, None, 1.0)
    n, mean, sd, _, _, _ = M.stats(0.0, [0.1] * 10 + [1e-17])
    assert mean == math.fsum([0.1] * 10 + [1e-17]) / 11 and sd > 0
    assert M.batch_fits(100, 30000) and not M.batch_fits(2, 1 << 62) and not M.batch_fits(1 << 31, 1)


# ------------------------------------------------------------------------------------------ the module on an oracle engine
class _NullEngine(_Engine):
    """test_regions_cpu's oracle engine plus null_batch on the numpy generator."""
    batches = []

    def null_batch(self, lens, seed, order):
        from frisk_amd import nullmodel as M
        sym, _ = self.profile
        _NullEngine.batches.append((list(lens), seed, order))
        self.load(M.generate_batch(sym, self.kmin, order, seed, lens))


@pytest.fixture
def fake_regions(monkeypatch):
    from frisk_amd import hotpath, regions
    monkeypatch.setattr(hotpath, "Engine", _NullEngine)
    real_init = hotpath.HotPath.__init__

    def init(self, kMin, kMax, device=0, cache_dir=None, use_cache=True):
        real_init(self, kMin, kMax, device=device, cache_dir=None, use_cache=use_cache)      # (no packed-sequence cache: no device)
    monkeypatch.setattr(hotpath.HotPath, "__init__", init)
    monkeypatch.setattr(hotpath.HotPath, "NULL_CHUNK", 7)                                    # several scoring calls per run
    _Engine.adds = 0
    _NullEngine.batches = []
    return regions


def _inputs(tmp_path):
    import ranges_cases as R
    rng = np.random.default_rng(3)
    rnd = lambda n: R._bases(rng, n, 0.5).decode()        # noqa: E731
    chr1 = rnd(120) + "N" * 30 + rnd(50)
    fa = tmp_path / "g.fa"
    fa.write_text(">chr1 the first\n%s\n>tiny\nACGTTGCAacg\n" % chr1)
    bed = tmp_path / "r.bed"
    bed.write_text("chr1\t0\t100\tgeneA\ntiny\t5\t9\tzw\nchr1\t10\t110\tsame_length\nchr1\t115\t155\tgap\nchr1\t150\t200\tright\n"
                   "chr1\t0\t3\nchr1\t0\t200\twhole\nchr1\t0\t60\tleft\n")
    return str(fa), str(bed), chr1


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [l.split("\t") for l in lines[1:-1]]


def _oracle_kld(seq, prof, kmin, kmax):
    """(KLD, valid) of one sequence as a region: valid = its row would carry note `.`."""
    enc = N.Encoded(seq)
    if enc.n - int(enc.upper.sum()) >= 0.3 * enc.n:
        return float("nan"), False
    hp = H.score_hp(enc, prof, kmin, kmax)
    return (float(hp["kld"]), True) if hp["flag"] == H.OK else (float("nan"), False)


HEADER = ["name", "start", "stop", "length", "id", "windowKLD", "nullN", "nullMean", "nullSD", "excess", "z", "p", "note"]


@pytest.mark.parametrize("mode", ["markov", "host"])
def test_module_end_to_end_with_a_null(fake_regions, tmp_path, mode):
    from frisk_amd import nullmodel as M
    from frisk_amd import postprocess as pp
    fa, bed, chr1 = _inputs(tmp_path)
    out = tmp_path / "t"
    argv = ["-H", fa, "-k", "4", "-t", str(out), "--bed", bed]
    assert fake_regions.main(argv) == 0
    plain = (out / "region_scores.tsv").read_bytes()
    assert not (out / "region_null_scores.tsv").exists()
    draws, seed = 9, 3
    assert fake_regions.main(argv + ["--null", mode, "--nullDraws", str(draws), "--seed", str(seed), "--recalc"]) == 0
    assert (out / "region_scores.tsv").read_bytes() == plain                # -O: byte for byte
    head, rows = _table(out / "region_null_scores.tsv")
    _, scored = _table(out / "region_scores.tsv")
    assert head == HEADER and len(rows) == 8
    assert [r[4] for r in rows] == ["geneA", "zw", "same_length", "gap", "right", ".", "whole", "left"]     # input order
    for r, s in zip(rows, scored):
        assert r[:4] == s[:4] and r[5] == s[4] and r[12] == s[7]            # windowKLD and note as -O prints them
    assert [r[12] for r in rows] == [".", "ZeroDivisionError", ".", "unresolved", ".", "noMaxmer", ".", "."]
    for r in rows:
        if r[12] != ".":
            assert r[6:12] == ["."] * 6
    # every draw again, from the numpy generator / the host's slices and the oracle on each
    seqs = [chr1, "ACGTTGCAacg"]
    prof = N.genome_profile(seqs, 1, 4)
    lengths = sorted({int(r[3]) for r in rows if r[12] == "."})
    assert lengths == [50, 60, 100, 200]
    if mode == "markov":
        assert _NullEngine.batches == [([200] * draws, seed, 3)]            # one batch, the longest length, order kmax - 1
        batch = M.generate_batch(prof[0], 1, 3, seed, [200] * draws)
        null = {L: [_oracle_kld(b[:L], prof, 1, 4) for b in batch] for L in lengths}
    else:
        assert _NullEngine.batches == []
        null = {L: [_oracle_kld(seqs[s][a:a + L], prof, 1, 4) for s, a in M.host_draws([200, 11], L, draws, seed)] for L in lengths}
        assert len(null[200]) == draws and {d for d in M.host_draws([200, 11], 200, draws, seed)} == {(0, 0)}
    fmt = pp.py2_str
    close = lambda a, b: abs(float(a) - b) <= 1e-9 * max(1.0, abs(b))      # noqa: E731  (the text has 12 digits)
    for r in rows:
        if r[12] != ".":
            continue
        v = [k for k, ok in null[int(r[3])] if ok]
        own, ok = _oracle_kld(chr1[int(r[1]) - 1:int(r[2])], prof, 1, 4)   # (in full precision: a tie is a tie)
        assert ok and r[5] == fmt(own)
        n, mean, sd, excess, z, p = M.stats(own, v)
        assert r[6] == str(n) and n >= 1
        assert close(r[7], mean) and close(r[9], excess)
        assert (r[8] == ".") == (sd is None) and (sd is None or close(r[8], sd))
        assert (r[10] == ".") == (z is None)
        assert r[11] == fmt(p)
    if mode == "host":
        whole = [r for r in rows if r[4] == "whole"][0]                     # one start position: every draw is the region itself
        assert whole[6] == str(draws) and whole[11] == "1.0" and whole[10] == "." and float(whole[8]) == 0.0
        gene = [r for r in rows if r[4] == "geneA"][0]
        assert 1 <= int(gene[6]) < draws                                    # slices over the N run are dropped as the region would be
    # the same seed gives the same file, another seed another
    first = (out / "region_null_scores.tsv").read_bytes()
    again = argv + ["--null", mode, "--nullDraws", str(draws), "--nullOutfile", "again.tsv"]
    assert fake_regions.main(again + ["--seed", str(seed)]) == 0 and (out / "again.tsv").read_bytes() == first
    assert fake_regions.main(again + ["--seed", "4"]) == 0
    assert (out / "again.tsv").read_bytes() != first


def test_null_order_and_a_query_without_a_long_enough_host(fake_regions, tmp_path):
    from frisk_amd import nullmodel as M
    fa, bed, chr1 = _inputs(tmp_path)
    out = tmp_path / "t"
    assert fake_regions.main(["-H", fa, "-m", "2", "-k", "4", "-t", str(out), "--bed", bed, "--null", "markov", "--nullDraws", "2",
                              "--nullOrder", "1"]) == 0
    assert _NullEngine.batches == [([200, 200], 0, 1)]                      # --seed defaults to 0
    # a query longer than every host scaffold: no host slice of the region's length
    import ranges_cases as R
    q = tmp_path / "q.fa"
    q.write_text(">q\n%s\n" % R._bases(np.random.default_rng(5), 300, 0.5).decode())
    qbed = tmp_path / "q.bed"
    qbed.write_text("q\t0\t250\tlong\nq\t0\t40\tshort\n")
    assert fake_regions.main(["-H", fa, "-Q", str(q), "-k", "4", "-t", str(out), "--bed", str(qbed), "--null", "host",
                              "--nullDraws", "3"]) == 0
    _, rows = _table(out / "region_null_scores.tsv")
    assert rows[0][12] == "." and rows[0][6:12] == ["."] * 6
    assert rows[1][12] == "." and rows[1][6] in ("1", "2", "3") and rows[1][11] != "."
    assert M.host_draws([200, 11], 250, 3, 0) == []
    # an empty input: the header alone
    empty = tmp_path / "empty.bed"
    empty.write_text("# nothing\n")
    assert fake_regions.main(["-H", fa, "-k", "4", "-t", str(out), "--bed", str(empty), "--null", "host", "--nullOutfile", "e.tsv"]) == 0
    assert (out / "e.tsv").read_text() == "\t".join(HEADER) + "\n"


def test_refusals_come_before_any_device_work(fake_regions, tmp_path, caplog):
    fa, bed, _ = _inputs(tmp_path)
    out = tmp_path / "t"
    base = ["-H", fa, "-k", "4", "-t", str(out), "--bed", bed]
    huge = tmp_path / "huge.bed"
    huge.write_text("chr1\t0\t%d\n" % (1 << 62))
    donor = tmp_path / "d.fa"
    donor.write_text(">d\nACGTACGTTGCA\n")
    for extra, word in ((["--null", "markov", "--donors", str(donor)], "--null does not go with --donors"),
                        (["--null", "host", "--nullDraws", "0"], "--nullDraws"),
                        (["--null", "markov", "--nullDraws", "-3"], "--nullDraws"),
                        (["--null", "markov", "--nullOrder", "4"], "--nullOrder"),
                        (["--null", "markov", "--nullOrder", "-1"], "--nullOrder"),
                        (["--null", "markov", "-m", "3", "--nullOrder", "1"], "--nullOrder"),
                        (["--null", "host", "--nullOrder", "3"], "--nullOrder"),
                        (["--null", "markov", "--nullDraws", "2"], "--nullDraws")):
        caplog.clear()
        argv = (base[:-1] + [str(huge)] if extra[-1] == "2" else base) + extra
        assert fake_regions.main(argv) == 1, extra
        assert word in caplog.text, (extra, caplog.text)
        assert _Engine.adds == 0 and _NullEngine.batches == [] and not (out / "region_scores.tsv").exists()
    with pytest.raises(SystemExit):
        fake_regions.build_parser().parse_args(base + ["--null", "shuffle"])
    # without --null the other options change nothing
    assert fake_regions.main(base + ["--nullDraws", "0", "--nullOrder", "99"]) == 0
    assert not (out / "region_null_scores.tsv").exists()
