"""Host model of svo_trace_instances and svo_trace_instance_shadows (include/svo.h).  Test infrastructure of tests/test_instances.py
and tests/test_instances_cpu.py.

Both stages are specified in separately rounded float, so the model repeats them in numpy float32: the transform into an instance's
space, the box rule, the pairs, their ranks, the cap and the drop; the model rays are marched by the unchanged CPU oracle
(ow.trace_rays) and the far end is applied by segments_model.expected; then the resolve, stage 2's two lists and its fold.  The
methods of Model are the places where the CPU tests plant their mutations; the model never overrides them.

Also the scene of the GPU tests: the model grid, the eight instances and the statistics their floors are asserted on.
"""
import numpy as np

import local_shadows_model as M
import segments_model as SEG

F = np.float32
HIT, TRACED, SHADOWED, FACE, ERR = 1, 2, 4, 8, 1 << 15
MAX_INSTANCES = 32
INF = F(np.inf)


# ---- instances ---------------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    """Rodrigues' matrix in float64, rounded once to float32: what the svo_instance holds."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + s * K + (1 - c) * (K @ K)).astype(F)


def instance(pos, scale=1.0, rot=None):
    """(rot float32[3, 3], pos float32[3], scale float32): one placement, x_world = pos + scale * (R x_model)."""
    return (np.eye(3, dtype=F) if rot is None else np.asarray(rot, F).reshape(3, 3), np.asarray(pos, F), F(scale))


def centred(centre, scale=1.0, rot=None, model_centre=(16.0, 16.0, 16.0)):
    """The placement that puts the model's centre at `centre`: pos = centre - scale * R c (float64, rounded once)."""
    R = np.eye(3) if rot is None else np.asarray(rot, np.float64).reshape(3, 3)
    pos = np.asarray(centre, np.float64) - float(scale) * (R @ np.asarray(model_centre, np.float64))
    return instance(pos.astype(F), scale, rot)


def instance_structs(svo, instances):
    return [svo.Instance(R.reshape(-1), pos, float(scale)) for R, pos, scale in instances]


def world_box(chunkcoordmin, dims, chunksize):
    """(bmin, bmax) of a world as floats: chunkcoordmin * chunksize, and that plus dims * chunksize."""
    ccm, dims = np.asarray(chunkcoordmin, np.int64), np.asarray(dims, np.int64)
    return (ccm * chunksize).astype(F), ((ccm + dims) * chunksize).astype(F)


def shadow_direction(light_dir=(1.0, -1.0, 0.0)):
    """normalize(-light_dir) as the library's host code forms it, in float32."""
    n = -np.asarray(light_dir, F)
    inv = F(1.0) / np.sqrt(F(F(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
    return (n * inv).astype(F)


# ---- the two steps every pair goes through -----------------------------------------------------------------------------
def to_model(o, d, inst):
    """(om, dm) float32 [n, 3]: om[i] = ((R[0][i]*u.x + R[1][i]*u.y) + R[2][i]*u.z) * inv with u = o - pos, dm likewise without inv."""
    R, pos, scale = inst
    inv = F(1.0) / F(scale)
    with np.errstate(all="ignore"):
        u = (o - pos[None, :]).astype(F)
        d = np.broadcast_to(np.asarray(d, F), u.shape)
        om = np.stack([(((R[0, i] * u[:, 0] + R[1, i] * u[:, 1]) + R[2, i] * u[:, 2]) * inv) for i in range(3)], axis=1)
        dm = np.stack([((R[0, i] * d[:, 0] + R[1, i] * d[:, 1]) + R[2, i] * d[:, 2]) for i in range(3)], axis=1)
    assert om.dtype == F and dm.dtype == F
    return om, dm


class Model:
    def box_rule(self, om, dm, box):
        """(missed, tn): the header's step 2, per axis in x, y, z order."""
        bmin, bmax = box
        n = om.shape[0]
        tn, tf, fail = np.zeros(n, F), np.full(n, INF, F), np.zeros(n, bool)
        with np.errstate(all="ignore"):
            for a in range(3):
                o, g = om[:, a], dm[:, a]
                flat = g == 0
                fail |= flat & ~((bmin[a] <= o) & (o <= bmax[a]))
                r = (F(1.0) / g).astype(F)
                t0, t1 = ((bmin[a] - o) * r).astype(F), ((bmax[a] - o) * r).astype(F)
                swap = t1 < t0
                t0, t1 = np.where(swap, t1, t0), np.where(swap, t0, t1)
                tn = np.where(~flat & (t0 > tn), t0, tn)
                tf = np.where(~flat & (t1 < tf), t1, tf)
            return fail | (tn > tf), tn

    def before(self, tn, far):
        with np.errstate(invalid="ignore"):
            return tn < far

    def ranks(self, pair):
        """pair[ninst, n] -> the rank of every pair (garbage elsewhere): instance-major, ascending pixel within an instance."""
        flat = pair.reshape(-1)
        return (np.cumsum(flat) - flat).reshape(pair.shape)

    def nearer(self, tw, best):
        return tw < best                                    # ties go to the lowest j

    # ---- stage 1 -------------------------------------------------------------------------------------------------------
    def trace(self, oracle, om_world, box, cam, rect, gbuffer, instances, semantics=0, max_rays=0, eps=0.0, normal_mode=0):
        """What svo_trace_instances leaves for `gbuffer` (the records of the rectangle): dict(merged, owner uint32[n], counts (pairs,
        min(pairs, cap)), cap, pair, slot - the rank where the pair has a slot, -1 elsewhere -, hitting[ninst, n], stats)."""
        g = np.asarray(gbuffer).reshape(-1)
        n = g.shape[0]
        o, d = M.camera_rays(oracle, cam, rect)
        sel = M.usable(g)
        ninst = len(instances)
        pair, rays = np.zeros((ninst, n), bool), []
        for j, inst in enumerate(instances):
            om, dm = to_model(o, d, inst)
            missed, tn = self.box_rule(om, dm, box)
            with np.errstate(all="ignore"):
                far = np.where(sel, (g["t"].astype(F) * (F(1.0) / F(inst[2]))).astype(F), INF).astype(F)
            pair[j] = ~missed & self.before(tn, far)
            rays.append((om, dm, far))
        cap = max_rays if max_rays > 0 else n
        rank = self.ranks(pair)
        total = int(pair.sum())
        marched = pair & (rank < cap)
        params = oracle.make_params(shadow=False, semantics=semantics, eps=eps, normal_mode=normal_mode)
        merged, owner = np.array(g, copy=True), np.zeros(n, np.uint32)
        best, found = np.zeros(n, F), np.zeros(n, bool)
        hitting, stats = np.zeros((ninst, n), bool), []
        for j, (R, pos, scale) in enumerate(instances):
            om, dm, far = rays[j]
            go = marched[j]
            raw = om_world.trace_rays(om[go], dm[go], params=params, threads=8) if go.any() else np.zeros(0, g.dtype)
            rec = SEG.expected(raw, far[go])
            hit = M.usable(rec)
            hitting[j][go] = hit
            tw = np.zeros(n, F)
            tw[go] = (rec["t"].astype(F) * F(scale)).astype(F)
            win = hitting[j] & (~found | self.nearer(tw, best))
            full = np.zeros(n, g.dtype)
            full[go] = rec
            nm = full["normal"].astype(F)
            with np.errstate(invalid="ignore"):
                nw = np.stack([((R[i, 0] * nm[:, 0] + R[i, 1] * nm[:, 1]) + R[i, 2] * nm[:, 2]) for i in range(3)], axis=1).astype(F)
            merged["t"][win] = tw[win]
            merged["normal"][win] = nw[win]
            for f in ("material", "chunk", "node", "cell"):
                merged[f][win] = full[f][win]
            merged["flags"][win] = HIT | (full["flags"][win] & FACE)
            owner[win] = j + 1
            best, found = np.where(win, tw, best), found | win
            stats.append(dict(pairs=int(pair[j].sum()), dropped=int((pair[j] & ~marched[j]).sum()), hitting=int(hitting[j].sum()),
                              lost_to_scene=int((M.usable(raw) & ~hit).sum()), runaways=int(np.count_nonzero(raw["flags"] & ERR))))
        for j in range(ninst):
            stats[j]["owned"] = int((owner == j + 1).sum())
        return dict(merged=merged, owner=owner, counts=(total, min(total, cap)), cap=cap, pair=pair, slot=np.where(marched, rank, -1), hitting=hitting,
                    stats=stats, contested=int((hitting.sum(axis=0) >= 2).sum()))

    # ---- stage 2 -------------------------------------------------------------------------------------------------------
    def shadows(self, oracle, scene_world, om_world, box, cam, rect, merged, owner, instances, semantics=0, max_rays=0, bias=0.0, eps=0.0,
                light_dir=(1.0, -1.0, 0.0)):
        """What svo_trace_instance_shadows leaves of `merged` / `owner` (stage 1's): dict(merged, counts, cap, pair, considered, by_model,
        by_scene - which considered pixels the model list / the scene list occluded -, self_at_zero - per instance the pixels it owns and
        occludes at t = 0 -, runaways)."""
        m = np.array(merged, copy=True).reshape(-1)
        n = m.shape[0]
        owner = np.asarray(owner, np.uint32).reshape(-1)
        o, d = M.camera_rays(oracle, cam, rect)
        S = shadow_direction(light_dir)
        b = F(bias) if bias > 0 else M.resolved_eps(semantics, eps)
        considered = M.usable(m) & ((m["flags"] & SHADOWED) == 0)
        with np.errstate(all="ignore"):
            P = M.sample_points(o, d, m, b)
        ninst = len(instances)
        pair, rays = np.zeros((ninst, n), bool), []
        for j, inst in enumerate(instances):
            om, dm = to_model(P, S[None, :], inst)
            missed, _ = self.box_rule(om, dm, box)
            pair[j] = considered & ~missed
            rays.append((om, dm))
        cap = max_rays if max_rays > 0 else n
        rank = self.ranks(pair)
        total = int(pair.sum())
        marched = pair & (rank < cap)
        params = oracle.make_params(shadow=False, semantics=semantics, eps=eps)
        by_model, self_zero, runaways = np.zeros(n, bool), [], 0
        for j in range(ninst):
            om, dm = rays[j]
            go = marched[j]
            rec = om_world.trace_rays(om[go], dm[go], params=params, threads=8) if go.any() else np.zeros(0, m.dtype)
            occ = np.zeros(n, bool)
            occ[go] = M.usable(rec)
            zero = np.zeros(n, bool)
            zero[go] = M.usable(rec) & (rec["t"] == 0)
            by_model |= occ
            self_zero.append(int((zero & (owner == j + 1)).sum()))
            runaways += int(np.count_nonzero(rec["flags"] & ERR))
        go = considered & (owner != 0)
        rec = scene_world.trace_rays(P[go], np.broadcast_to(S, (int(go.sum()), 3)), params=params, threads=8) if go.any() else np.zeros(0, m.dtype)
        by_scene = np.zeros(n, bool)
        by_scene[go] = M.usable(rec)
        runaways += int(np.count_nonzero(rec["flags"] & ERR))
        m["flags"] = np.where(considered, m["flags"] | TRACED | np.where(by_model | by_scene, SHADOWED, 0), m["flags"]).astype(m["flags"].dtype)
        return dict(merged=m, counts=(total, min(total, cap)), cap=cap, pair=pair, considered=considered, by_model=by_model, by_scene=by_scene,
                    self_at_zero=self_zero, runaways=runaways)


MODEL = Model()
trace = MODEL.trace
shadows = MODEL.shadows


# ---- the scene of tests/test_instances.py ------------------------------------------------------------------------------
MODEL_DEPTH, MODEL_SIZE = 5, 32
BIAS = 1.0 / 256.0


def model_grid():
    """A [z, y, x] grid of 32^3 cells: a hollow ball shell (radius 9.5 to 14.5 cells about the centre) of material 3 with a band of
    material 5 round its middle, a round hole through the +x side and a slot through the top, so that rays enter, pass through and
    self-shadow."""
    z, y, x = np.meshgrid(*(np.arange(32) + 0.5,) * 3, indexing="ij")
    r = np.sqrt((x - 16) ** 2 + (y - 16) ** 2 + (z - 16) ** 2)
    g = np.where((r >= 9.5) & (r <= 14.5), 3, 0).astype(np.uint16)
    g[(g != 0) & (np.abs(y - 16) < 3)] = 5
    g[(x > 16) & ((y - 16) ** 2 + (z - 16) ** 2 < 25)] = 0
    g[(y > 16) & (np.abs(x - 14) < 2.5) & (np.abs(z - 16) < 7)] = 0
    return g


EYE, FORWARD, RIGHT = (128.0, 150.0, -40.0), (0.0, -0.5, 0.866), (-1.0, 0.0, 0.0)      # svo.default_camera(2, 2, 128, ...)
VISIBLE, HIDDEN, AROUND_EYE, OFF_SCREEN = (0, 1, 2, 3, 5, 6), 4, 6, 7


def scene_instances():
    """The eight placements in World.generate(2, 1, 2, 128, 8) under default_camera(2, 2, 128, 128, 96); the light comes from -x, above.
      0  identity, at an integer position, in the air in front of the hill
      1  about y by 30 degrees, scale 1.5, over the lit water east of the hill: its shadow falls on the water
      2  about the skew axis (1, 2, 3) by 40 degrees, scale 0.5, in the air near the camera
      3  about z by 90 degrees, scale 2.5, half buried in the water that the western slope shadows
      4  identity, inside the hill: corners of its box stick out, so it has pairs, and it owns nothing
      5  about x by 20 degrees, scale 1.25, behind instance 0 and to its side: the two overlap on screen
      6  about y by 45 degrees, around the eye: every pixel is a pair that starts inside the box (tn = 0), the ball shows at one edge
      7  behind the camera: no pairs"""
    e, f, r = (np.asarray(v, np.float64) for v in (EYE, FORWARD, RIGHT))
    side = np.radians(78.0)
    return [instance((94.0, 84.0, 4.0)),
            centred((185.0, 45.0, 95.0), 1.5, rotation((0, 1, 0), 30.0)),
            centred((120.0, 115.0, 0.0), 0.5, rotation((1, 2, 3), 40.0)),
            centred((50.0, 6.0, 85.0), 2.5, rotation((0, 0, 1), 90.0)),
            centred((127.0, 40.0, 60.0)),
            centred((76.0, 75.0, 50.0), 1.25, rotation((1, 0, 0), 20.0)),
            centred(e + 21.0 * (np.sin(side) * r + np.cos(side) * f), 1.0, rotation((0, 1, 0), 45.0)),
            centred((128.0, 150.0, -140.0))]
