"""python -m frisk_amd.regions --null in fresh child processes on the device: markov_islands.fa with its hand-written annotation,
19 draws per length, both nulls.  -O is the file of the run without --null; the null table is reproducible and follows the seed;
and every draw is made again on the host - nullmodel's generator and host draws, the numpy oracle on each - so that nullN and p
must match exactly and the moments to 1e-10 (the table's text has 12 digits: that, not the kernel, limits the comparison)."""
import functools
import os
import subprocess
import sys

import pytest

import kld_oracle_hp as H
from golden_util import INPUTS
from oracle import frisk_oracle as O
from oracle import frisk_oracle_np as N

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FA = os.path.join(INPUTS, "markov_islands.fa")
GFF = os.path.join(INPUTS, "markov_islands.gff3")
DRAWS, SEED = 19, 3
HEADER = ["name", "start", "stop", "length", "id", "windowKLD", "nullN", "nullMean", "nullSD", "excess", "z", "p", "note"]


def _run(argv, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("FRISK_FLOAT_REPR", None)
    return subprocess.run([sys.executable, "-m", "frisk_amd.regions"] + argv, cwd=str(cwd), env=env, capture_output=True, text=True,
                          timeout=300)


def _records():
    from frisk_amd import regions
    names = [n for n, _ in O.iter_fasta(FA)]
    return [(names.index(n), a, b, ident) for n, a, b, ident in regions.read_gff_regions(GFF) if n in names]


def _score(seq, prof):
    """(KLD by the numpy oracle, its bound, note is `.`) of one sequence scored as a region at k = 1..8."""
    enc = seq if isinstance(seq, N.Encoded) else N.Encoded(seq)
    if enc.n - int(enc.upper.sum()) >= 0.3 * enc.n:
        return float("nan"), 0.0, False
    hp = H.score_hp(enc, prof, 1, 8)
    if hp["flag"] != H.OK:
        return float("nan"), 0.0, False
    row = N.score_window(enc, N.genome_ivom_table(prof[0], prof[1], 1, 8), 1, 8)
    return float(row["KLD"]), float(H.bound(hp["scale"])), True


@functools.lru_cache(maxsize=None)
def expected(mode, seed=SEED):
    """Per record of the annotation: None (its note is not `.`) or (KLD, bound, [(KLD, bound) of each valid draw])."""
    from frisk_amd import nullmodel as M
    seqs = H.read_fasta(FA)
    prof = H.profile(seqs, 1, 8)
    recs = _records()
    own = [_score(N.Encoded(seqs[s]).slice(a, b), prof) for s, a, b, _ in recs]
    lengths = sorted({b - a for (s, a, b, _), o in zip(recs, own) if o[2]})
    if mode == "markov":
        batch = M.generate_batch(prof[0], 1, 7, seed, [max(lengths)] * DRAWS)
        draws = {L: [_score(x[:L], prof) for x in batch] for L in lengths}
    else:
        encs = [N.Encoded(x) for x in seqs]
        draws = {L: [_score(encs[s].slice(a, a + L), prof) for s, a in M.host_draws([len(x) for x in seqs], L, DRAWS, seed)]
                 for L in lengths}
    return [(o[0], o[1], [(k, bd) for k, bd, ok in draws[b - a] if ok]) if o[2] else None for (s, a, b, _), o in zip(recs, own)]


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [l.split("\t") for l in lines[1:-1]]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The run without --null (it also leaves the genome k-mer cache and the packed-sequence cache for the others)."""
    cwd = tmp_path_factory.mktemp("null_cli")
    gff = cwd / "on_the_fasta.gff3"             # the annotation without the record on chrM, which the FASTA does not hold
    gff.write_text("".join(l for l in open(GFF) if not l.startswith("chrM")))
    p = _run(["-H", FA, "-t", "out", "--gff", str(gff)], cwd)
    assert p.returncode == 0, p.stderr
    return cwd, str(gff), (cwd / "out" / "region_scores.tsv").read_bytes()


_FIRST = {}


def _first(plain, mode):
    """The run with --seed SEED in this mode, made once: (argv without the seed, its null table's bytes)."""
    cwd, gff, _ = plain
    argv = ["-H", FA, "-t", "out", "--gff", gff, "--null", mode, "--nullDraws", str(DRAWS), "--nullOutfile", mode + ".tsv"]
    if mode not in _FIRST:
        p = _run(argv + ["--seed", str(SEED)], cwd)
        assert p.returncode == 0, p.stderr
        _FIRST[mode] = (cwd / "out" / (mode + ".tsv")).read_bytes()
    return argv, _FIRST[mode]


@pytest.mark.parametrize("mode", ["markov", "host"])
def test_null_table_against_the_host_side_draws(plain, mode):
    from frisk_amd import nullmodel as M
    from frisk_amd import postprocess as pp
    cwd, gff, scores = plain
    exp = expected(mode)
    # the oracle's own values first: no draw within the two bounds of its region's score (p would hang on the last bits)
    for e in exp:
        if e is not None:
            assert all(abs(k - e[0]) > bd + e[1] for k, bd in e[2]), e
    assert sum(e is not None for e in exp) >= 15 and all(len(e[2]) >= 2 for e in exp if e is not None)
    _first(plain, mode)
    assert (cwd / "out" / "region_scores.tsv").read_bytes() == scores                       # -O: byte for byte
    head, rows = _table(cwd / "out" / (mode + ".tsv"))
    _, scored = _table(cwd / "out" / "region_scores.tsv")
    assert head == HEADER and len(rows) == len(exp) == 21
    worst = 0.0
    for r, s, e, (_, a, b, ident) in zip(rows, scored, exp, _records()):
        assert r[:4] == s[:4] and r[1:5] == [str(a + 1), str(b), str(b - a), ident] and r[5] == s[4] and r[12] == s[7]
        if e is None:
            assert r[12] != "." and r[6:12] == ["."] * 6
            continue
        n, mean, sd, excess, z, pv = M.stats(e[0], [k for k, _ in e[2]])
        assert r[12] == "." and r[6] == str(n) and r[11] == pp.py2_str(pv), (r, n, pv)
        for got, want in zip(r[7:11], (mean, sd, excess, z)):
            err = abs(float(got) - want) / abs(want)
            worst = max(worst, err)
            assert err <= 1e-10, (r, got, want)
    print("%s null: %d records placed, worst relative error of the moments %.3g" % (mode, sum(e is not None for e in exp), worst))


@pytest.mark.parametrize("mode", ["markov", "host"])
def test_null_table_is_reproducible_and_follows_the_seed(plain, mode):
    cwd, _, scores = plain
    argv, first = _first(plain, mode)
    p = _run(argv[:-1] + ["again.tsv", "--seed", str(SEED)], cwd)
    assert p.returncode == 0 and (cwd / "out" / "again.tsv").read_bytes() == first
    p = _run(argv[:-1] + ["other.tsv", "--seed", str(SEED + 1)], cwd)
    assert p.returncode == 0 and (cwd / "out" / "other.tsv").read_bytes() != first
    assert (cwd / "out" / "region_scores.tsv").read_bytes() == scores
