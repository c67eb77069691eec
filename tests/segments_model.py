"""Host model of svo_trace_segments (include/svo.h): the call is DEFINED as a filter over what svo_trace_rays writes, so the unchanged
CPU oracle checks it - march the list with ow.trace_rays, keep record k iff it is a usable hit with t < tmax[k] (one float32
compare, strict), write the all-zero miss record otherwise.  Also the far-end inputs of tests/test_segments*.py."""
import numpy as np

HIT, ERR = 1, 1 << 15
F = np.float32
UNIFORM = 200.0                                              # the uniform far end of the scene (and the fill of near_ties)


def usable(records):
    f = records["flags"].reshape(-1)
    return ((f & HIT) != 0) & ((f & ERR) == 0)


def kept(records, tmax):
    """Which records survive: usable hits with t < tmax (NaN compares false)."""
    r = records.reshape(-1)
    tmax = np.broadcast_to(np.asarray(tmax, F), r.shape)
    with np.errstate(invalid="ignore"):
        return usable(r) & (r["t"].astype(F) < tmax)


def expected(records, tmax):
    """The records svo_trace_segments writes, from the unbounded ones of the same rays and params."""
    r = records.reshape(-1)
    out = np.zeros_like(r)
    k = kept(r, tmax)
    out[k] = r[k]
    return out


def uniform(records, value=UNIFORM):
    return np.full(records.reshape(-1).shape[0], value, F)


def near_ties(records, fill=UNIFORM):
    """tmax[k] = the unbounded t of ray k - 1 (`fill` where that ray has no usable hit, and for ray 0): neighbouring pixels hit at
    nearly the same distance, and sometimes at exactly the same."""
    r = records.reshape(-1)
    t = np.where(usable(r), r["t"].astype(F), F(fill)).astype(F)
    out = np.full(r.shape[0], fill, F)
    out[1:] = t[:-1]
    return out


def half_way(records):
    """tmax[k] = 0.5 * t of the unbounded hit, +inf where the ray has none: every hit is dropped, its march can stop half way."""
    r = records.reshape(-1)
    return np.where(usable(r), F(0.5) * r["t"].astype(F), F(np.inf)).astype(F)


def shares(records, tmax):
    """(hits, kept, dropped, exact ties) of the usable hits under tmax."""
    r = records.reshape(-1)
    u, k = usable(r), kept(r, tmax)
    tmax = np.broadcast_to(np.asarray(tmax, F), r.shape)
    return int(u.sum()), int(k.sum()), int((u & ~k).sum()), int((u & (r["t"].astype(F) == tmax)).sum())
