"""SKL-TSNE on the GPU against tests/golden/skltsne.json + skltsne/skltsne.npz (sklearn 1.7's own functions, recorded on the CPU by
tools/make_skltsne_golden.py).  Neither sklearn nor the reference is read here.

Bounds.  Each is C x eps x scale with C = 4 x the worst deviation, over all golden cases, of sklearn's recorded value from a long
double restatement of the same formula with direct-difference distances (tests/skltsne_oracle.py), the factor 4 standing for the
device's different summation order (the C_KLD precedent of tests/kld_oracle_hp.py).  The constants live in the json
("calibration"); as recorded, with the worst value the CPU measured and the worst the device showed on an MI355X, in the same units:

    quantity                      eps    scale                      worst CPU   C        worst device
    dense joint P                 eps64  row maximum of P           17.4        69.6     9.57
    sparse conditional P          eps64  row maximum of p_j|i       4.60        18.4     3.31
    gradient, exact               eps32  max |grad|                 0.593       2.37     0 (read off the update: bit-identical)
    gradient, barnes_hut          eps32  max |grad|                 76.8        307      78.5 (read off the update)
    error, exact                  eps64  sum |terms| + sum P        1.08        4.31     2.61
    error, barnes_hut             eps32  sum |terms| + sum P        26.5        106      26.5

(barnes_hut: sklearn accumulates forces and error in float32, the device in FP64, so the device's distance from sklearn is
sklearn's own from the long double.  The error's scale includes sum P because p / Q carries a relative rounding error that the
logarithm turns into an absolute one: a term errs by p x a few eps however small log(p / Q) is.  A first calibration against
sum |terms| alone gave C = 23.6, which the device missed at one state, 44.8 at n = 3 near its optimum, where every ratio is close to
1 and sum |terms| is a hundredth of sum P; on the scale above that state sits at 0.49.)
No float32-rounded distance of any golden case differs between sklearn's expansion form and the direct differences (the tool counted
0 flipped entries, dense and sparse), so the P bounds carry no allowance for a flip.  beta and the bisection's step count are exact
results of the same decisions and are compared for equality.
The gains rule is discontinuous in the sign of update x grad: where |grad| is within the gradient bound of 0 the device may
take the other branch, so there a gain may be either of the rule's two values, and the update bound uses the larger.
The short horizon (iterations 0 .. 10) is chaotic already: a perturbation of the size of the per-step gradient bound at every step
moves sklearn's own trajectory by 1.46 (exact) and 2.46 (barnes_hut) x max |Y| over 8 draws; the bound is 4 x that, so this test
mostly guards against a blow-up.  The init='pca' start is within 4 x the measured deviation of sklearn's randomized start from the
exact one (0.54 of the 1e-4 scale, worst of 8 seeds)."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import skltsne_oracle as O
from frisk_amd import _ffi
from frisk_amd import projection as P

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "skltsne.json")) as _fh:
    M = json.load(_fh)
_G = None
CAL = {k: v["C"] for k, v in M["calibration"].items()}
EPS64, EPS32 = O.EPS64, O.EPS32
WORST = {}


def G(key):
    global _G
    if _G is None:
        _G = np.load(os.path.join(GOLD, "skltsne", "skltsne.npz"))
    return _G[key]


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def cases(prefix):
    return sorted(k for k in M if k.startswith(prefix))


def inputs(m):
    return O.make_X(m["seed"], m["n"], m["f"], m.get("kind", "dirichlet"))


# ------------------------------------------------------------------------------------------------ affinities
@pytest.mark.parametrize("name", cases("dense_"))
def test_dense_affinities(name):
    m = M[name]
    n = m["n"]
    with P.SKLTSNE(inputs(m), 2, m["perplexity"], "exact") as h:
        beta, steps = h.affinities()
        Pd = h.p_dense()
    assert np.array_equal(steps, G(name + "/steps"))
    assert np.array_equal(beta, G(name + "/beta"))
    assert np.array_equal(Pd, Pd.T) and not Pd.diagonal().any()
    rowmax = G(name + "/rowmax")
    if m["whole"]:
        rows, want = np.arange(n), G(name + "/P")
    else:
        rows, want = G(name + "/rows"), G(name + "/P_rows")
    dev = np.max(np.abs(Pd[rows] - want) / rowmax[rows, None]) / EPS64
    note("P_dense", dev)
    print(name, "dense P: %.3g eps64 of the row maximum (bound %.3g)" % (dev, CAL["P_dense"]))
    assert dev <= CAL["P_dense"]
    # every row, through its sum: n entries, each within the bound
    assert np.all(np.abs(Pd.sum(axis=1) - G(name + "/rowsum")) <= n * CAL["P_dense"] * EPS64 * rowmax)


def test_constructed_rows_run_all_steps_and_none():
    assert np.all(G("dense_n2_f44/steps") == 100) and np.all(G("dense_simplex8/steps") == 0)      # (compared above)


@pytest.mark.parametrize("name", cases("sparse_"))
def test_sparse_affinities(name):
    m = M[name]
    n, k = m["n"], m["k"]
    with P.SKLTSNE(inputs(m), 2, m["perplexity"], "barnes_hut") as h:
        assert h.k == k
        beta, steps = h.affinities()
        idx, cond = h.neighbours()
    assert np.array_equal(steps, G(name + "/steps"))
    assert np.array_equal(beta, G(name + "/beta"))
    if m["whole"]:
        rows, want_idx, want = np.arange(n), G(name + "/idx"), G(name + "/cond")
    else:
        rows, want_idx, want = G(name + "/rows"), G(name + "/idx_rows"), G(name + "/cond_rows")
    assert np.array_equal(idx[rows], want_idx)
    assert np.all(np.diff(idx, axis=1) > 0) and idx.min() >= 0 and idx.max() < n and not np.any(idx == np.arange(n)[:, None])
    dev = np.max(np.abs(cond[rows] - want) / want.max(axis=1)[:, None]) / EPS64
    note("P_sparse", dev)
    print(name, "conditional P: %.3g eps64 of the row maximum (bound %.3g)" % (dev, CAL["P_sparse"]))
    assert dev <= CAL["P_sparse"]
    assert np.all(np.abs(cond.sum(axis=1) - 1.0) <= k * CAL["P_sparse"] * EPS64)
    # the host symmetrisation: the pattern is sklearn's, the values (a + b) / S with a, b within the bound and S = 2 n
    J = P.skl_tsne_joint_nn(idx, cond)
    assert np.array_equal(np.diff(J.indptr), G(name + "/joint_nnz"))
    per_entry = 2 * CAL["P_sparse"] * cond.max() / (2.0 * n)
    row_sums = G(name + "/joint_rowsum")
    assert np.all(np.abs(np.asarray(J.sum(axis=1)).ravel() - row_sums) <= (n * per_entry + 4 * n * row_sums) * EPS64)
    if m["whole"]:
        assert np.array_equal(J.indptr, G(name + "/joint_indptr")) and np.array_equal(J.indices, G(name + "/joint_indices"))
        want = G(name + "/joint_data")
        assert np.all(np.abs(J.data - want) <= (per_entry + 4 * want) * EPS64)


# ------------------------------------------------------------------------------------------------ single steps
def handle(m):
    X = O.make_X(m["seed"], m["n"], m["f"])
    h = P.SKLTSNE(X, m["d"], m["perplexity"], m["method"])
    h.affinities()
    if m["method"] == "barnes_hut":
        h.set_p(P.skl_tsne_joint_nn(*h.neighbours()))
    return h


def check_step(name, m, step, before, after, grad, rows, got, err, norm):
    _Y0, U0, G0 = before
    n, d = m["n"], m["d"]
    Cg = CAL["grad_" + m["method"]]
    tol_g = Cg * EPS32 * step["gmax"]
    both = (np.maximum(G0 + np.float32(0.2), np.float32(0.01)), np.maximum(G0 * np.float32(0.8), np.float32(0.01)))
    sure = np.abs(grad) > tol_g
    gY, gU, gG = (a[rows] for a in got)
    assert np.array_equal(gG[sure], after[2][sure]), name
    assert np.all((gG == both[0][rows]) | (gG == both[1][rows])), name
    top = np.maximum(both[0], both[1])[rows]
    tol_u = 1000.0 * tol_g * top + 4 * EPS32 * (np.abs(after[1]) + np.abs(U0[rows]))
    dev_u = np.max(np.abs(gU.astype(np.float64) - after[1]) / (1000.0 * top)) / (EPS32 * step["gmax"])
    note("grad_" + m["method"], dev_u)
    assert np.all(np.abs(gU.astype(np.float64) - after[1]) <= tol_u), (name, step, dev_u)
    assert np.all(np.abs(gY.astype(np.float64) - after[0]) <= tol_u + 2 * EPS32 * np.abs(after[0])), (name, step)
    eps = EPS64 if m["method"] == "exact" else EPS32
    dev_e = abs(err - step["error"]) / step["err_scale"] / eps
    note("err_" + m["method"], dev_e)
    assert dev_e <= CAL["err_" + m["method"]], (name, step, dev_e)
    tol_n = np.sqrt(n * d) * tol_g * float(np.max(both[0])) + 4 * EPS32 * step["grad_norm"]
    assert abs(norm - step["grad_norm"]) <= tol_n, (name, step, norm)
    print(name, step.get("from", step.get("state")), "update %.3g eps32 gmax (C %.3g), error %.3g eps (C %.3g)"
          % (dev_u, Cg, dev_e, CAL["err_" + m["method"]]))


@pytest.mark.parametrize("name", cases("gd_"))
def test_one_step_from_every_recorded_state(name):
    m = M[name]
    assert m["steps"], name
    with handle(m) as h:
        for step in m["steps"]:
            if "state" in step:
                before = O.synthetic_state(step["state_seed"], m["n"], m["d"], step["state"])
                rows = np.array(step["rows"])
                after = tuple(G("%s/%s_after_%s" % (name, step["state"], c)) for c in "YUG")
                grad = G("%s/%s_grad" % (name, step["state"]))
                it = 0 if step["state"] == "start" else 250
            else:
                it = step["from"]
                before = tuple(G("%s/s%d_%s" % (name, it, c)) for c in "YUG")
                after = tuple(G("%s/s%d_%s" % (name, step["to"], c)) for c in "YUG")
                grad = G("%s/s%d_grad" % (name, it))
                rows = np.arange(m["n"])
            h.set(*before)
            err, norm = h.run(it, it + 1, step["momentum"], step["exaggeration"])
            check_step(name, m, step, before, after, grad, rows, h.get(), err, norm)


@pytest.mark.parametrize("method", ["exact", "barnes_hut"])
def test_ten_steps_in_one_run_equal_ten_runs_and_runs_repeat(method):
    name = "gd_%s_n65_d2" % method
    m = M[name]
    start = tuple(G("%s/s0_%s" % (name, c)) for c in "YUG")
    out = []
    for split in (False, True, False):
        with handle(m) as h:
            h.set(*start)
            if split:
                for i in range(10):
                    last = h.run(i, i + 1, 0.5, 4.0)
            else:
                last = h.run(0, 10, 0.5, 4.0)
            out.append((h.get(), last))
    for other in out[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(out[0][0], other[0]))
        assert out[0][1] == other[1]


@pytest.mark.parametrize("method", ["exact", "barnes_hut"])
def test_short_horizon(method):
    name = "gd_%s_n65_d2" % method
    m = M[name]
    with handle(m) as h:
        h.set(*(G("%s/s0_%s" % (name, c)) for c in "YUG"))
        h.run(0, 11, 0.5, 4.0)
        Y = h.get()[0]
    ref = G(name + "/s11_Y")
    dev = np.max(np.abs(Y - ref)) / np.max(np.abs(ref))
    print(name, "iterations 0..10: %.3g of max |Y| (bound %.3g)" % (dev, 4 * m["horizon_dev"]))
    assert np.all(np.isfinite(Y)) and dev <= 4 * m["horizon_dev"]


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("method, ensemble", [("exact", "exact"), ("barnes_hut", "barnes_hut_angle0")])
def test_full_run_lies_in_sklearns_ensemble(method, ensemble):
    e = M["e2e"]
    X = O.make_X(e["seed"], e["n"], e["f"])
    res = P.skl_tsne(X, 2, e["perplexity"], seed=0, method=method)
    kls, its = e["ensembles"][ensemble]["kl_divergence"], e["ensembles"][ensemble]["n_iter"]
    spread = max(kls) - min(kls)
    print(method, "n_iter", res.n_iter, "KL", res.kl_divergence, "sklearn", sorted(set(its)), min(kls), max(kls))
    assert res.Y.dtype == np.float32 and res.Y.shape == (e["n"], 2) and np.all(np.isfinite(res.Y))
    assert min(kls) - spread <= res.kl_divergence <= max(kls) + spread
    assert any(abs(res.n_iter - i) in (0, 50) for i in its)
    assert np.array_equal(res.Y0, O.random_start(0, e["n"], 2))
    assert res.kl_divergence == res.errors[-1] and res.n_iter == res.check_iters[-1]


def test_pca_start_is_sklearns_up_to_the_randomized_solver():
    e = M["e2e"]
    X = O.make_X(e["seed"], e["n"], e["f"])
    Y0 = P.skl_tsne_start(X, 2, np.random.RandomState(0), "pca")
    dev = np.max(np.abs(Y0 - G("e2e/Y0_pca_sklearn"))) / 1e-4
    print("pca start: %.3g of 1e-4 (bound %.3g)" % (dev, 4 * e["pca_start_dev"]))
    assert Y0.dtype == np.float32 and dev <= 4 * e["pca_start_dev"]
    res = P.skl_tsne(X[:80], 3, 10.0, seed=1, method="exact", init="pca")
    assert res.Y.shape == (80, 3) and np.all(np.isfinite(res.Y)) and np.isfinite(res.kl_divergence)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kwargs", [dict(perplexity=30.0), dict(dims=4, method="barnes_hut"), dict(method="tree"), dict(init="x")])
def test_argument_errors_come_before_any_device_call(monkeypatch, kwargs):
    def no_device(*_a, **_k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(P, "SKLTSNE", no_device)
    monkeypatch.setattr(P, "pca", no_device)
    with pytest.raises(ValueError):
        P.skl_tsne(np.zeros((30, 5)), **kwargs)
    with pytest.raises(ValueError):
        P.skl_tsne(np.zeros((1, 5)))


def test_abi_refusals():
    X = O.make_X(1, 10, 4)
    for dims, perp, method in ((2, 10.0, "exact"), (4, 3.0, "barnes_hut"), (0, 3.0, "exact"), (65, 3.0, "exact")):
        with pytest.raises(_ffi.FriskHipError) as err:
            P.SKLTSNE(X, dims, perp, method)
        assert err.value.code == _ffi.E_ARG
    with P.SKLTSNE(X, 2, 3.0, "barnes_hut") as h:
        with pytest.raises(_ffi.FriskHipError) as err:
            h.run(0, 1, 0.5, 4.0)                       # no joint probabilities yet
        assert err.value.code == _ffi.E_STATE
        with pytest.raises(_ffi.FriskHipError) as err:
            h.p_dense()
        assert err.value.code == _ffi.E_STATE
        h.affinities()
        J = P.skl_tsne_joint_nn(*h.neighbours())
        bad = J.copy()
        bad.indices = bad.indices.copy()
        bad.indices[0] = 10                              # a column out of range never reaches the device
        with pytest.raises(_ffi.FriskHipError) as err:
            h.set_p(bad)
        assert err.value.code == _ffi.E_ARG
        h.set_p(J)
        with pytest.raises(_ffi.FriskHipError):
            h.run(5, 5, 0.5, 4.0)
        with pytest.raises(_ffi.FriskHipError):
            h.run(0, 1001, 0.5, 4.0)
        err_, norm = h.run(0, 1, 0.5, 4.0)
        assert np.isfinite(err_) and np.isfinite(norm)


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra, label", [((), "barnes_hut, init random"),
                                          (("--tsneGradient", "exact", "--tsneInitPCA", "pca"), "exact, init pca")])
def test_cli_runs_the_projection_and_dumps_it(tmp_path, extra, label):
    """python -m frisk_amd --runProjection SKL-TSNE on the projection fixture (198 anomalous windows x 44 proportions): the run logs
    iterations and KL divergence instead of "not built here", writes the embedding with --dumpPCAdata, and - --cluster being still
    fenced - keeps the warning and writes no cluster GFF3."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = ["-m", "1", "-k", "4", "-w", "200", "-i", "100", "-F", "0.1991", "--runProjection", "SKL-TSNE", "--pcaMin", "1", "--pcaMax", "3",
            "--cluster", "KMEANS", "--gffOutfile", "a.gff3", "--dumpPCAdata", "--seed", "3"] + list(extra)
    cmd = [sys.executable, "-m", "frisk_amd", "-H", os.path.join(GOLD, "inputs", "proj_islands.fa"), "-t", str(tmp_path)] + argv
    p = subprocess.run(cmd, cwd=repo, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "SKL-TSNE (%s) of 198 x 44 k-mer proportions:" % label in p.stderr and "KL divergence" in p.stderr
    assert "is not built here" not in p.stderr and "--cluster is not available in this build" in p.stderr
    with open(tmp_path / "anomSKLTSNE", "rb") as fh:
        Y = pickle.load(fh)
    assert Y.shape == (198, 2) and Y.dtype == np.float32 and np.all(np.isfinite(Y))
    files = sorted(os.listdir(tmp_path))
    assert "a.gff3" in files and "anomCounts" in files and not [f for f in files if "cluster_labeled" in f]


def test_zz_report():
    print("worst device deviations:", json.dumps(WORST, sort_keys=True))
