"""The input envelope of the numerical features (numpy only): the families of non-finite and out-of-range rows that the
feature-envelope tests plant into ordinary batches, and the float64 statement of the numerical preprocessing.

The 13 numerical features are the only continuous values that reach the kernels from outside the process, so these are the
rows a caller can actually send: a NaN or an infinity in one feature or in all, rows scaled far out of the N(0, 1) range
the rest of the suite draws, and the zeros / tiny values / negative zeros at the other end.  Magnitudes between 2^60 and
overflow are left out: there the float32 reference itself overflows and disagrees with float64.
"""
import numpy as np

# family -> (what bad_rows writes).  The first four make the reference return NaN for the whole row (pinned by
# tests/golden/envelope_<case>.npz); the others stay finite in float32 and float64.
NONFINITE = ("nan_one", "pinf_one", "ninf_one", "nan_all")
FINITE = ("x2p20", "x2p40", "one_2p60", "zeros", "tiny", "negzero")
FAMILIES = NONFINITE + FINITE
ORDINARY = "ordinary"


def plant(row, family, col):
    """One float32 feature row of ``family``, made from the ordinary row ``row`` (``col``: the feature the single-feature
    families write)."""
    r = np.array(row, dtype=np.float32, copy=True)
    if family == "nan_one":
        r[col] = np.nan
    elif family == "pinf_one":
        r[col] = np.inf
    elif family == "ninf_one":
        r[col] = -np.inf
    elif family == "nan_all":
        r[:] = np.nan
    elif family == "x2p20":
        r *= np.float32(2.0 ** 20)
    elif family == "x2p40":
        r *= np.float32(2.0 ** 40)
    elif family == "one_2p60":
        r[col] = np.float32(2.0 ** 60)
    elif family == "zeros":
        r[:] = 0.0
    elif family == "tiny":
        r[:] = np.float32(1e-30)
    elif family == "negzero":
        r[:] = -0.0
    else:
        raise KeyError(family)
    return r


def bad_rows(un, positions, families=FAMILIES):
    """-> (copy of ``un`` [B, n] with the i-th of ``positions`` replaced by a row of family ``families[i % len]``, made
    from the row it replaces; the family of every row, ORDINARY where nothing was planted).  The single-feature families
    write feature ``position % n``, so the planted feature moves across the columns with the row."""
    un = np.asarray(un, dtype=np.float32)
    out = un.copy()
    fam = [ORDINARY] * un.shape[0]
    for i, p in enumerate(positions):
        p = int(p)
        assert 0 <= p < un.shape[0] and fam[p] == ORDINARY, (p, un.shape[0])
        fam[p] = families[i % len(families)]
        out[p] = plant(un[p], fam[p], p % un.shape[1])
    return out, fam


def rows_of(fam, which):
    """Boolean row mask of the families in ``which`` (a name or a tuple of names)."""
    which = (which,) if isinstance(which, str) else tuple(which)
    return np.array([f in which for f in fam], dtype=bool)


def prep_reference(x32, mean32, scale32):
    """(log1p(|x|) - mean) / scale in float64 from the float32 inputs (amdrec_prep_numerical's contract; mean and scale
    per column, broadcast over the rows)."""
    x = np.abs(np.asarray(x32, dtype=np.float32).astype(np.float64))
    with np.errstate(all="ignore"):
        return (np.log1p(x) - np.asarray(mean32, dtype=np.float32).astype(np.float64)) \
            / np.asarray(scale32, dtype=np.float32).astype(np.float64)
