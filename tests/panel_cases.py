"""The profiles of the frisk_score_ranges_panel tests  --  TEST INFRASTRUCTURE.

The ranges are the range set of tests/ranges_cases.py.  A panel of P profiles: donor p is one seeded scaffold of 150 000 bases
whose GC content rises with p; the last slot is always the scaffolds' own profile (R.profile).  Profiles come from
kld_oracle_hp.profile as (sym, meta)."""
import functools

import numpy as np

import kld_oracle_hp as H
import ranges_cases as R
from oracle import frisk_oracle_np as N

DONOR_BASES = 150000


@functools.lru_cache(maxsize=None)
def donor(p, P):
    return R._bases(np.random.default_rng(700 + p), DONOR_BASES, 0.25 + 0.5 * p / max(P - 1, 1))


@functools.lru_cache(maxsize=None)
def profiles(P, kmin, kmax):
    """The P profiles of a panel, in slot order: P - 1 donors, then the scaffolds' own."""
    return tuple(H.profile([donor(p, P)], kmin, kmax) for p in range(P - 1)) + (R.profile(kmin, kmax),)


def install(engine, prof):
    sym, meta = prof
    engine.profile_set(sym, *[int(v) for v in meta])


@functools.lru_cache(maxsize=None)
def expected(P, kmin, kmax):
    """(rows, [oracle rows of plane p]) of the range set under each profile of the panel, computed once."""
    rows = R.range_set(kmax)
    out = []
    for sym, meta in profiles(P, kmin, kmax):
        ig = N.genome_ivom_table(sym, meta, kmin, kmax)
        out.append(R.expect_rows(R.scaffolds(), (sym, meta), ig, rows, kmin, kmax))
    return rows, out
