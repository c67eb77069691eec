"""Host models of svo_trace_lights and svo_shade_lights (include/svo.h).  Test infrastructure of tests/test_lights.py and
tests/test_lights_cpu.py.

The trace model is built from tests/local_shadows_model.py (camera_rays, sample_points, light_rays, usable) plus the reach and
facing tests in numpy float32; the rays are marched by the unchanged CPU oracle (ow.trace_rays), and the rank, cap and drop rule is
applied here.  The methods of TraceModel are the places where the CPU tests plant their mutations; the model never overrides them.

The shading model is float64, written from the header in the style of tests/shade_model.py, and is judged with that file's `within`.
"""
import numpy as np

import local_shadows_model as M
import shade_model as sm

F = np.float32
MAX_LIGHTS = 32
# the scene of tests/test_lights.py, World.generate(2, 1, 2, 128, 8) under default_camera(2, 2, 128, 128, 96): (position, reach)
LIGHTS = [((50.0, 8.0, 65.0), 64.0), ((50.0, 20.0, 70.0), 96.0), ((128.0, 120.0, 128.0), 200.0), ((100.0, 40.0, 160.0), 80.0),
          ((180.0, 60.0, 90.0), 100.0), ((64.5, 3.0, 64.5), 40.0), ((100.3, 40.0, 100.3), 60.0), ((-300.0, 400.0, -200.0), 1000.0),
          ((128.0, 30.0, 128.0), 24.0), ((90.0, 25.0, 110.0), 48.0)]


def light_vectors(P, position):
    """v = L - P and q = (v.x*v.x + v.y*v.y) + v.z*v.z in float32, as local_shadows_model.light_rays makes them."""
    with np.errstate(all="ignore"):
        v = (np.asarray(position, F)[None, :] - P).astype(F)
        q = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F)
    assert v.dtype == F and q.dtype == F
    return v, q


class TraceModel:
    def in_reach(self, q, R2):
        with np.errstate(invalid="ignore"):
            return q <= R2

    def facing(self, s):
        with np.errstate(invalid="ignore"):
            return ~(s <= 0)                                 # a NaN s faces the light

    def ranks(self, pair):
        """pair[nlights, n] -> the rank of every pair (garbage elsewhere): light-major, ascending pixel within a light."""
        flat = pair.reshape(-1)
        return (np.cumsum(flat) - flat).reshape(pair.shape)

    def dropped_visible(self):
        return True                                         # a pair without a slot is not marched and counts as not occluded

    def pairs(self, P, normals, sel, lights):
        """(pair[nlights, n], in reach but culled as back-facing [nlights, n], dirs, dist per light)"""
        n = P.shape[0]
        pair, back, rays = np.zeros((len(lights), n), bool), np.zeros((len(lights), n), bool), []
        for j, (position, reach) in enumerate(lights):
            v, q = light_vectors(P, position)
            valid, dirs, dist = M.light_rays(P, position)
            with np.errstate(all="ignore"):
                R2 = F(reach) * F(reach)
                s = ((normals[:, 0] * v[:, 0] + normals[:, 1] * v[:, 1]) + normals[:, 2] * v[:, 2]).astype(F)
            near = sel & valid & self.in_reach(q, R2)
            pair[j] = near & self.facing(s)
            back[j] = near & ~pair[j]
            rays.append((dirs, dist))
        return pair, back, rays

    def trace(self, oracle, ow, cam, rect, frame, lights, semantics=0, max_rays=0, eps=0.0):
        """What svo_trace_lights leaves for `frame` (the records of the rectangle): dict(words uint32[n], counts (pairs, min(pairs,
        cap)), cap, pair, slot - the pair's rank where it has a slot, -1 elsewhere -, stats - per light: pairs, occluded, visible,
        backfacing, dropped, runaways, nearest |t - dist| / dist)."""
        rec = np.asarray(frame).reshape(-1)
        n = rec.shape[0]
        o, d = M.camera_rays(oracle, cam, rect)
        sel = M.usable(rec)
        P = M.sample_points(o, d, rec, M.resolved_eps(semantics, eps))
        pair, back, rays = self.pairs(P, rec["normal"].astype(F), sel, lights)
        cap = max_rays if max_rays > 0 else n
        rank = self.ranks(pair)
        total = int(pair.sum())
        marched = pair & (rank < cap)
        words = np.zeros(n, np.uint32)
        stats = []
        params = oracle.make_params(shadow=False, semantics=semantics, eps=eps)
        for j in range(len(lights)):
            dirs, dist = rays[j]
            go = marched[j]
            r = ow.trace_rays(P[go], dirs[go], params=params, threads=8) if go.any() else np.zeros(0, sm.HIT_DTYPE)
            hit = M.usable(r)
            occ = np.zeros(n, bool)
            occ[go] = hit & (r["t"] < dist[go])
            vis = (marched[j] & ~occ) | ((pair[j] & ~marched[j]) if self.dropped_visible() else False)
            words |= np.where(vis, np.uint32(1 << j), np.uint32(0)).astype(np.uint32)
            with np.errstate(all="ignore"):
                near = np.abs(r["t"].astype(np.float64) - dist[go]) / dist[go]
            stats.append(dict(pairs=int(pair[j].sum()), occluded=int(occ.sum()), visible=int((marched[j] & ~occ).sum()), backfacing=int(back[j].sum()),
                              dropped=int((pair[j] & ~marched[j]).sum()), runaways=int(np.count_nonzero(r["flags"] & M.ERR)),
                              nearest=float(near[hit].min()) if hit.any() else float("inf")))
        return dict(words=words, counts=(total, min(total, cap)), cap=cap, pair=pair, slot=np.where(marched, rank, -1), stats=stats,
                    usable=int(sel.sum()), P=P)


MODEL = TraceModel()
trace = MODEL.trace


def light_structs(svo, lights, colours=None):
    """svo.Light per (position, reach); colours: per light (ambient, diffuse, specular, attenuation), default a white lamp."""
    out = []
    for j, (position, reach) in enumerate(lights):
        amb, dif, spe, att = colours[j] if colours is not None else ((0.05, 0.05, 0.05), (0.8, 0.8, 0.8), (1.0, 1.0, 1.0), (1.0, 0.09, 0.032))
        out.append(svo.Light(position, reach, amb, dif, spe, att))
    return out


# ---- svo_shade_lights, float64 -----------------------------------------------------------------------------------------
def shade_lights(cam, P, rect, g, lights, words=None, model=sm.MODEL):
    """(add[n, 3], cond[n], ratio[nlights, n]): the sum over the lights of C_j for every record with SVO_HIT_FLAG (0 for the others),
    cond = shininess * sum over the lights of max_c |specular term after att and vis|, and d / reach.  `lights` are svo.Light;
    words: uint32[n] (None: every light unshadowed)."""
    g = np.asarray(g).reshape(-1)
    n = g.shape[0]
    T = model.terms(cam, P, rect, g)
    p, vdir, shin = T["p"], T["vdir"], T["shininess"]
    gam = model.gamma(float(P.gamma) or float(np.float32(2.2)))
    mi = model.material_index(g["material"].astype(np.int64))
    with np.errstate(invalid="ignore"):
        diffuse = np.array([list(m.diffuse) for m in P.materials], np.float64)[mi] ** gam
        specular = np.array([list(m.specular) for m in P.materials], np.float64)[mi] ** gam
    nrm = g["normal"].astype(np.float64)
    hit = (g["flags"] & sm.HIT) != 0
    words = np.full(n, 0xFFFFFFFF, np.uint32) if words is None else np.asarray(words, np.uint32)
    add, cond, ratio = np.zeros((n, 3)), np.zeros(n), np.zeros((len(lights), n))
    for j, L in enumerate(lights):
        reach = float(L.reach)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            lv = sm._v(L.position) - p
            d = np.sqrt(sm._dot(lv, lv))
            l = lv / d[:, None]
            hv = sm._unit(l + vdir)
            win = np.clip(1.0 - (d / reach) ** 4, 0.0, 1.0) ** 2
            att = (win / (float(L.constant) + float(L.linear) * d + float(L.quadratic) * d * d))[:, None]
            vis = ((words >> np.uint32(j)) & np.uint32(1)).astype(np.float64)[:, None]
            amb = sm._v(L.ambient) * diffuse
            dif = sm._v(L.diffuse) * sm._max0(sm._dot(nrm, l))[:, None] * diffuse * vis
            spe = sm._v(L.specular) * model.power(sm._max0(sm._dot(vdir, hv)), shin)[:, None] * specular * vis
            c = ((amb + dif) + spe) * att
            inside = hit & (d > 0.0) & (d < reach)
        add += np.where(inside[:, None], c, 0.0)
        with np.errstate(invalid="ignore"):
            cond += np.where(inside, shin * np.nan_to_num(np.abs(spe * att).max(axis=1), nan=0.0, posinf=0.0), 0.0)
        ratio[j] = np.where(hit, d / reach, np.nan)
    return add, cond, ratio
