"""SKL-TSNE without a GPU: the ABI's names, the CLI wiring (with projection.skl_tsne replaced), the host stop rule
(projection.skl_tsne_descent) against sklearn's recorded check sequences and hand-made ones, and the oracle's transcription of
_gradient_descent against sklearn's own loop."""
import json
import logging
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import skltsne_oracle as O
from frisk_amd import _ffi, cli
from frisk_amd import projection as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["frisk_skltsne_create", "frisk_skltsne_affinities", "frisk_skltsne_p_dense", "frisk_skltsne_neighbours", "frisk_skltsne_set_p",
         "frisk_skltsne_get", "frisk_skltsne_set", "frisk_skltsne_run", "frisk_skltsne_last_ms", "frisk_skltsne_destroy"]


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "skltsne.json")) as fh:
        return json.load(fh)


def test_abi_names_are_declared_and_bound():
    bound = {s[0] for s in _ffi.SYMBOLS}
    with open(os.path.join(ROOT, "include", "frisk_hip.h")) as fh:
        header = fh.read()
    for name in NAMES:
        assert name in bound, name
        assert name + "(" in header, name


def test_analysis_unit_includes_the_kernels_after_spectral():
    with open(os.path.join(ROOT, "frisk_amd", "csrc", "frisk_analysis.hip")) as fh:
        src = fh.read()
    assert '#include "skltsne_kernels.h"' in src
    assert src.index('#include "spectral_kernels.h"') < src.index('#include "skltsne_kernels.h"')
    with open(os.path.join(ROOT, "frisk_amd", "csrc", "skltsne_kernels.h")) as fh:
        kernels = fh.read()
    assert "namespace frisk_skltsne_impl" in kernels and "atomicAdd" not in kernels


def test_projection_tuples():
    assert cli.PROJECTIONS_DUMPED == ("SKL-TSNE",)
    assert "SKL-TSNE" not in cli.PROJECTIONS and cli.PROJECTIONS_UNCLUSTERED == ("NMF",)
    args = cli.build_parser().parse_args(["-H", "g.fa", "--runProjection", "SKL-TSNE", "--cluster", "KMEANS"])
    assert ("cluster", "sklearn clustering is out of scope") in cli.unavailable(args)


class _Clock:
    def lap(self, _name):
        pass


def _args(tmp_path, *extra):
    return cli.build_parser().parse_args(["-H", "g.fa", "-t", str(tmp_path), "--runProjection", "SKL-TSNE"] + list(extra))


@pytest.mark.parametrize("extra, want", [
    ((), dict(method="barnes_hut", init="random", perplexity=20.0, seed=0, dims=2)),
    (("--tsneGradient", "exact", "--tsneInitPCA", "pca", "--perplexity", "7.5", "--seed", "11", "--projectionDims", "3",
      "--cluster", "DBSCAN", "--gffOutfile", "a.gff3"), dict(method="exact", init="pca", perplexity=7.5, seed=11, dims=3)),
])
@pytest.mark.parametrize("dump", [False, True])
def test_project_calls_skl_tsne_with_the_cli_options(tmp_path, monkeypatch, extra, want, dump):
    X = np.arange(12.0).reshape(4, 3)
    Y = np.ones((4, want["dims"]), dtype=np.float32)
    seen = {}

    def fake(X_, dims, perplexity, seed, method, init, device):
        seen.update(X=X_, dims=dims, perplexity=perplexity, seed=seed, method=method, init=init, device=device)
        return SimpleNamespace(Y=Y, n_iter=349, kl_divergence=2.5, timings={"affinities_ms": 1.0, "init_ms": 2.0, "iterations_ms": 3.0})
    monkeypatch.setattr(P, "skl_tsne", fake)
    args = _args(tmp_path, *(extra + (("--dumpPCAdata",) if dump else ())))
    assert cli._project(args, X, 0, _Clock()) is None
    assert seen.pop("X") is X and seen.pop("device") == 0
    assert seen == want
    path = os.path.join(str(tmp_path), "anomSKLTSNE")
    assert os.path.exists(path) == dump
    if dump:
        with open(path, "rb") as fh:
            assert np.array_equal(pickle.load(fh), Y)
    assert [f for f in os.listdir(str(tmp_path)) if f != "anomSKLTSNE"] == []       # no cluster GFF3, nothing else


def test_a_value_error_is_a_warning(tmp_path, monkeypatch, caplog):
    def refuse(*_a, **_k):
        raise ValueError("perplexity must be less than n_samples")
    monkeypatch.setattr(P, "skl_tsne", refuse)
    with caplog.at_level(logging.WARNING, logger="frisk"):
        assert cli._project(_args(tmp_path, "--dumpPCAdata"), np.zeros((3, 2)), 0, _Clock()) is None
    assert any("SKL-TSNE skipped" in r.getMessage() and "perplexity" in r.getMessage() for r in caplog.records)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("kwargs, text", [
    (dict(n=20, perplexity=20.0), "perplexity must be less than n_samples"),
    (dict(dims=4, method="barnes_hut"), "should be inferior to 4"),
    (dict(n=1), "between 2 and 50000"), (dict(n=50001), "between 2 and 50000"),
    (dict(method="tree"), "method"), (dict(init="spectral"), "init"), (dict(dims=0), "n_components"),
])
def test_argument_errors(kwargs, text):
    a = dict(n=100, f=44, dims=2, perplexity=20.0, method="barnes_hut", init="random")
    a.update(kwargs)
    with pytest.raises(ValueError, match=text):
        P.skl_tsne_check(**a)
    P.skl_tsne_check(100, 44, 4, 20.0, "exact", "pca")          # dims = 4 is the exact method's to take


# ------------------------------------------------------------------------------------------------ the stop rule
class Replay:
    """A handle whose run() answers from recorded checks {iteration: (error, norm)}; any other last iteration gets `other`."""

    def __init__(self, checks, other=(1.0, 1.0)):
        self.checks, self.other, self.calls = {int(c[0]): (c[1], c[2]) for c in checks}, other, []

    def run(self, begin, end, momentum, exaggeration):
        self.calls.append((begin, end, momentum, exaggeration))
        return self.checks.get(end - 1, self.other)


def _sequences(meta):
    for name, m in sorted(meta.items()):
        if name.startswith("gd_") and "n_iter" in m:
            yield name, m
    for method, m in sorted(meta["e2e"]["transcribed"].items()):
        yield "e2e_" + method, m


def test_descent_reproduces_sklearns_n_iter_on_every_recorded_sequence(meta):
    count = 0
    for name, m in _sequences(meta):
        h = Replay(m["checks_stage1"] + m["checks_stage2"])
        kl, n_iter, checks = P.skl_tsne_descent(h)
        assert n_iter == m["n_iter"], name
        assert kl == m["kl_divergence"], name
        assert [c[0] for c in checks] == [c[0] for c in m["checks_stage1"] + m["checks_stage2"]], name
        # contiguous, in order, 50 at a time at the most, stage 1 exaggerated with momentum 0.5
        assert all(b[0] == a[1] for a, b in zip(h.calls, h.calls[1:])) and all(e - b <= 50 for b, e, _m, _x in h.calls), name
        stage2 = m["checks_stage1"][-1][0] + 1               # (250, or earlier where stage 1 stopped on the norm)
        assert all((mo, ex) == ((0.5, 4.0) if b < stage2 else (0.8, 1.0)) for b, _e, mo, ex in h.calls), name
        count += 1
    assert count >= 10


def test_grad_norm_stop():
    h = Replay([(49, 3.0, 1e-7)])
    kl, n_iter, checks = P.skl_tsne_descent(h)            # stage 1 stops at 49 on the norm; stage 2 starts at 50 and meets its first
    assert h.calls[0] == (0, 50, 0.5, 4.0) and h.calls[1] == (50, 100, 0.8, 1.0)      # check at 99
    h = Replay([(49, 3.0, 1e-7), (99, 2.0, 1.0000001e-7), (149, 1.0, 1e-7)])
    kl, n_iter, _c = P.skl_tsne_descent(h)
    assert (kl, n_iter) == (1.0, 149)


def test_stage_one_never_stops_on_progress():
    checks = [(i, 5.0 + i, 1.0) for i in range(49, 250, 50)]        # the error only grows: i - best_iter is 200 at the most
    h = Replay(checks + [(299, 0.5, 1.0), (349, 0.6, 1.0)])
    _kl, n_iter, _c = P.skl_tsne_descent(h)
    assert [c[:2] for c in h.calls[:5]] == [(0, 50), (50, 100), (100, 150), (150, 200), (200, 250)] and n_iter == 349


def test_progress_edge_at_30_and_31():
    # with a check every 50 iterations i - best_iter is a multiple of 50; the edge itself needs other check intervals
    def run(interval, patience):
        errs = {interval - 1: 1.0}
        h = Replay([(i, errs.get(i, 2.0), 1.0) for i in range(interval - 1, 400, interval)])
        return P.skl_tsne_descent(h, max_iter=400, exploration=interval, n_iter_check=interval, n_iter_without_progress=patience)[1]
    # stage 2 starts at `interval` with best_iter = interval; its first check (2 interval - 1) sets best_iter, the next is interval later
    assert run(30, 30) == 30 * 4 - 1        # 30 > 30 is false at the second check: it goes on to the third (60 > 30)
    assert run(31, 30) == 31 * 3 - 1        # 31 > 30 stops at the second check of stage 2
    assert run(31, 31) == 31 * 4 - 1


def test_last_iteration_reads_the_error():
    checks = [(i, 10.0 - 0.001 * i, 1.0) for i in range(49, 1000, 50)]
    h = Replay(checks)
    kl, n_iter, _c = P.skl_tsne_descent(h)
    assert n_iter == 999 and kl == 10.0 - 0.001 * 999 and h.calls[-1][:2] == (950, 1000)
    h = Replay(checks, other=(7.0, 1.0))                        # a cap that is no check iteration: the last run ends there all the same
    kl, n_iter, _c = P.skl_tsne_descent(h, max_iter=980)
    assert (kl, n_iter) == (7.0, 979) and h.calls[-1][:2] == (950, 980)


# ------------------------------------------------------------------------------------------------ the oracle
def test_transcription_equals_sklearns_gradient_descent():
    T = pytest.importorskip("sklearn.manifold._t_sne")
    from sklearn.metrics import pairwise_distances
    X = O.make_X(465, 65, 44)
    Pc = T._joint_probabilities(pairwise_distances(X, metric="euclidean", squared=True), 20.0, 0) * 4.0
    Y0 = O.random_start(602, 65, 2)
    kw = dict(it=0, max_iter=250, n_iter_check=50, n_iter_without_progress=250, momentum=0.5, learning_rate=1000.0,
              min_grad_norm=1e-7, args=[Pc, 1, 65, 2], kwargs=dict(skip_num_points=0))
    p_sk, err_sk, it_sk = T._gradient_descent(T._kl_divergence, Y0.ravel(), **kw)
    p, err, it, _u, _g, checks = O.gradient_descent(T._kl_divergence, Y0.ravel(), 0, 250, 50, 250, 0.5, args=[Pc, 1, 65, 2],
                                                    kwargs=dict(skip_num_points=0))
    assert it == it_sk == 249 and err == err_sk and p.dtype == np.float32
    assert np.array_equal(p, p_sk)
    assert [c[0] for c in checks] == [49, 99, 149, 199, 249]
