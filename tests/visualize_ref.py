"""The two render specifications of the visualisation stage restated in pure PyTorch on the CPU, in fp32
or fp64 (tests only).  Built on the oracle's camera, pixel grid, pose and projection, which are imported and not edited.

Per pixel both functions return the winner id (-1: background), the winner's depth, the runner-up's depth (inf: none), the
decision margins and the float colour before quantisation, plus the quantised image.

`tol`: a surface is a CANDIDATE at a pixel when its hit margin is above -tol (primitives: 1 - m2, t_far - t_near; meshes:
the signed distance of the pixel centre to the nearest edge line, in NDC).  tol = 0 is the specification itself -- what a
kernel is compared against, in fp32.  The fp64 ambiguity analysis runs with tol = 1e-5: winner and runner-up are then taken
among everything that fp32 rounding could turn into a hit, and `ambiguous` marks the pixels where the answer hangs on
less than that: winner and runner-up depths within 1e-5 relative, or the margin of either within 1e-5 of zero."""
import math

import torch

from oracle import vpn_oracle as O

AMBIG = 1e-5
INF = float('inf')


def quantise(color):
    """ToPILImage after a clamp: [0,1] -> 0..255, truncated."""
    return (color.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def default_views(dist, elevs, azims):
    return [(dist, e, a) for a in azims for e in elevs]


def _pick(best, new, take):
    return [torch.where(take if b.dim() == take.dim() else take[..., None], n, b) for b, n in zip(best, new)]


def _two_nearest(z, cand, margin):
    """z, cand, margin [N,H,W] -> winner id, z1, margin1, z2, margin2 (first index wins equal depths)."""
    zc = torch.where(cand, z, torch.full_like(z, INF))
    z1, i1 = zc.min(0)                                                   # torch.min returns the first of equal minima
    hit = torch.isfinite(z1)
    m1 = torch.gather(margin, 0, i1[None])[0]
    zc2 = zc.clone()
    zc2.scatter_(0, i1[None], INF)
    z2, i2 = zc2.min(0)
    m2 = torch.gather(margin, 0, i2[None])[0]
    win = torch.where(hit, i1, torch.full_like(i1, -1))
    return win, z1, m1, z2, torch.where(torch.isfinite(z2), m2, torch.full_like(m2, INF))


def ref_primitives(params, kinds, cams, palette, H, W, ambient=1.0, background=(0.0, 0.0, 0.0), dtype=torch.float32, tol=0.0):
    """params [S,K,10], kinds list[K], cams [S,V,3], palette [>=K,3] -> dict of [S,V,H,W(,3)] tensors."""
    dt = dtype
    params, cams, palette = params.to(dt), cams.to(dt), palette.to(dt)
    S, K, _ = params.shape
    V = cams.shape[1]
    px, py = O.pixel_grid(H, W, dt)
    bg = torch.tensor(background, dtype=dt)
    is_box = torch.tensor([k == O.CUBOID for k in kinds])[:, None, None]
    out = {k: [] for k in ('winner', 'depth', 'runner', 'margin', 'runner_margin', 'color', 'base', 'cos')}
    for s in range(S):
        R = O.rotation_matrices(params[s, :, 3:7])                       # [K,3,3]
        Rt = R.transpose(1, 2)
        v, t = params[s, :, 0:3], params[s, :, 7:10]
        for vi in range(V):
            eye, right, up, fwd = (x[0] for x in O.camera_basis(cams[s, vi:vi + 1], dt))
            o = torch.einsum('kij,kj->ki', Rt, eye[None] - t) / v        # [K,3]
            Mr = torch.einsum('kij,j->ki', Rt, right) / v
            Mu = torch.einsum('kij,j->ki', Rt, up) / v
            Mf = torch.einsum('kij,j->ki', Rt, fwd) / v
            d = (Mf[:, None, None, :] + px[None, None, :, None] * Mr[:, None, None, :]) + py[None, :, None, None] * Mu[:, None, None, :]
            ob = o[:, None, None, :]
            dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
            ox, oy, oz = ob[..., 0], ob[..., 1], ob[..., 2]
            # ellipsoid
            A = (dx * dx + dy * dy) + dz * dz
            Bq = (ox * dx + oy * dy) + oz * dz
            ss = -Bq / A
            wx, wy, wz = ox + ss * dx, oy + ss * dy, oz + ss * dz
            u = 1.0 - ((wx * wx + wy * wy) + wz * wz)
            z_s = ss - torch.sqrt(u.clamp_min(0.0) / A)
            # cuboid: slab test on the unit box; tiny components as in oracle.raster
            sgn = torch.where(d < 0, -torch.ones_like(d), torch.ones_like(d))
            dsafe = torch.where(d.abs() < O.EPS_D, sgn * O.EPS_D, d)
            tn = (-sgn - ob) / dsafe
            tf = (sgn - ob) / dsafe
            ax = torch.where(tn[..., 1] > tn[..., 0], 1, 0)
            t_near = torch.where(tn[..., 1] > tn[..., 0], tn[..., 1], tn[..., 0])
            ax = torch.where(tn[..., 2] > t_near, 2, ax)
            t_near = torch.where(tn[..., 2] > t_near, tn[..., 2], t_near)
            t_far = torch.where(tf[..., 1] < tf[..., 0], tf[..., 1], tf[..., 0])
            t_far = torch.where(tf[..., 2] < t_far, tf[..., 2], t_far)
            margin = torch.where(is_box, t_far - t_near, u)
            z = torch.where(is_box, t_near, z_s)
            hit = torch.where(is_box, t_near <= t_far, u > 0) if tol == 0.0 else margin > -tol
            cand = hit & (z > O.MESH_NEAR)
            if tol != 0.0:                                               # the near plane is a margin too
                margin = torch.minimum(margin.abs(), (z - O.MESH_NEAR).abs())
            win, z1, m1, z2, m2 = _two_nearest(z, cand, margin)
            # colour of the winner
            kk = win.clamp_min(0)
            take = lambda x: torch.gather(x, 0, kk[None] if x.dim() == 3 else kk[None, ..., None].expand(1, H, W, x.shape[-1]))[0]
            dw = take(d)                                                 # [H,W,3]
            g_s = take(ob.expand_as(d)) + z1.nan_to_num(posinf=0.0)[..., None] * dw
            axw = take(ax)
            g_b = -take(sgn) * torch.nn.functional.one_hot(axw, 3).to(dt)
            g = torch.where(take(is_box.expand(K, H, W))[..., None], g_b, g_s)
            Rw, vw = R[kk], v[kk]                                        # [H,W,3,3], [H,W,3]
            gv = g / vw
            n = (Rw[..., :, 0] * gv[..., 0:1] + Rw[..., :, 1] * gv[..., 1:2]) + Rw[..., :, 2] * gv[..., 2:3]
            ray = (fwd[None, None, :] + px[None, :, None] * right[None, None, :]) + py[:, None, None] * up[None, None, :]
            nn = torch.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
            rn = torch.sqrt((ray[..., 0] * ray[..., 0] + ray[..., 1] * ray[..., 1]) + ray[..., 2] * ray[..., 2])
            cosv = -(((n[..., 0] * ray[..., 0] + n[..., 1] * ray[..., 1]) + n[..., 2] * ray[..., 2]) / (nn * rn))
            shade = ambient + (1.0 - ambient) * cosv.clamp_min(0.0)
            color = torch.where((win >= 0)[..., None], palette[kk] * shade[..., None], bg.expand(H, W, 3))
            for key, val in zip(('winner', 'depth', 'runner', 'margin', 'runner_margin', 'color', 'base', 'cos'),
                                (win, z1, z2, m1, m2, color, palette[kk], cosv.clamp_min(0.0))):
                out[key].append(val)
    return _finish(out, S, V, bg)


def _finish(out, S, V, bg):
    res = {k: torch.stack(vals).reshape((S, V) + vals[0].shape) for k, vals in out.items()}
    res['background'] = bg
    res['image'] = quantise(res['color'])
    res['ambiguous'] = _ambiguous(res)
    return res


def shaded_image(res, ambient):
    """The quantised image of a result at another `ambient` (winner, depths and margins do not depend on it)."""
    shade = ambient + (1.0 - ambient) * res['cos']
    color = torch.where((res['winner'] >= 0)[..., None], res['base'] * shade[..., None], res['background'].expand_as(res['base']))
    return quantise(color)


def _ambiguous(res):
    z1, z2 = res['depth'], res['runner']
    hit = res['winner'] >= 0
    tie = hit & torch.isfinite(z2) & ((z2 - z1).abs() < AMBIG * z1.abs())
    thin = (hit & (res['margin'].abs() < AMBIG)) | (torch.isfinite(z2) & (res['runner_margin'].abs() < AMBIG))
    return tie | thin


def ref_mesh(verts, faces, colors, cams, H, W, ambient=1.0, background=(0.0, 0.0, 0.0), dtype=torch.float32, tol=0.0, chunk=256):
    """verts [S,P,3], faces [F,3], colors [S,P,3], cams [S,V,3] -> the same dict; `margin` is the signed distance of the
    pixel centre to the nearest edge line of the winner (positive inside), in NDC."""
    dt = dtype
    verts, colors, cams = verts.to(dt), colors.to(dt), cams.to(dt)
    faces = faces.long()
    S, V, F = verts.shape[0], cams.shape[1], faces.shape[0]
    th = math.tan(0.5 * O.FOVY_DEG * math.pi / 180)
    px, py = O.pixel_grid(H, W, dt)
    gx = (px / th)[None, :].expand(H, W)
    gy = (py / th)[:, None].expand(H, W)
    bg = torch.tensor(background, dtype=dt)
    out = {k: [] for k in ('winner', 'depth', 'runner', 'margin', 'runner_margin', 'color', 'base', 'cos')}
    for s in range(S):
        for vi in range(V):
            cam = cams[s, vi:vi + 1]
            pr = O.mesh_project(verts[s:s + 1], cam)[0]                  # [P,3]
            eye, right, up, fwd = (x[0] for x in O.camera_basis(cam, dt))
            best = [torch.full((H, W), -1, dtype=torch.long), torch.full((H, W), INF, dtype=dt), torch.full((H, W), INF, dtype=dt),
                    torch.zeros(H, W, dtype=dt), torch.zeros(H, W, dtype=dt)]        # id, z, margin, weight a, weight b
            second = [torch.full((H, W), INF, dtype=dt), torch.full((H, W), INF, dtype=dt)]   # z, margin
            for f0 in range(0, F, chunk):
                fc = faces[f0:f0 + chunk]
                tri = pr[fc]                                             # [n,3,3]
                ok = (tri[..., 2] > O.MESH_NEAR).all(-1)[:, None, None]
                ax, ay, bx, by, cx, cy = (tri[:, i, j][:, None, None] for i in range(3) for j in range(2))
                iza, izb, izc = (1.0 / tri[:, i, 2][:, None, None] for i in range(3))
                e0 = (bx - ax) * (gy - ay) - (by - ay) * (gx - ax)
                e1 = (cx - bx) * (gy - by) - (cy - by) * (gx - bx)
                e2 = (ax - cx) * (gy - cy) - (ay - cy) * (gx - cx)
                area2 = (e0 + e1) + e2
                sg = torch.where(area2 < 0, -torch.ones_like(area2), torch.ones_like(area2))
                l0 = torch.sqrt((bx - ax) ** 2 + (by - ay) ** 2).clamp_min(1e-30)
                l1 = torch.sqrt((cx - bx) ** 2 + (cy - by) ** 2).clamp_min(1e-30)
                l2 = torch.sqrt((ax - cx) ** 2 + (ay - cy) ** 2).clamp_min(1e-30)
                margin = torch.minimum(torch.minimum(sg * e0 / l0, sg * e1 / l1), sg * e2 / l2)
                if tol == 0.0:
                    inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                else:
                    inside = margin > -tol
                cand = inside & (area2.abs() > O.MESH_MIN_AREA2) & ok
                wa, wb, wc = e1 / area2, e2 / area2, e0 / area2
                iz = (wa * iza + wb * izb) + wc * izc
                z = torch.where(cand, 1.0 / iz, torch.full_like(iz, INF))
                z = torch.where(torch.isnan(z), torch.full_like(z, INF), z)
                # nearest and second nearest of the chunk, then merged with the running ones (earlier faces win ties)
                zc1, j1 = z.min(0)
                pick = lambda x: torch.gather(x.expand_as(z), 0, j1[None])[0]
                c_id, c_m, c_wa, c_wb = j1 + f0, pick(margin), pick(wa), pick(wb)
                z_rest = z.clone()
                z_rest.scatter_(0, j1[None], INF)
                zc2, j2 = z_rest.min(0)
                c_m2 = torch.gather(margin.expand_as(z), 0, j2[None])[0]
                new_wins = zc1 < best[1]
                # the second place: the loser of (old best, chunk best) against (old second, chunk second)
                loser_z = torch.where(new_wins, best[1], zc1)
                loser_m = torch.where(new_wins, best[2], c_m)
                other_z = torch.where(zc2 < second[0], zc2, second[0])
                other_m = torch.where(zc2 < second[0], c_m2, second[1])
                second = [torch.where(loser_z <= other_z, loser_z, other_z), torch.where(loser_z <= other_z, loser_m, other_m)]
                best = _pick(best, [c_id, zc1, c_m, c_wa, c_wb], new_wins)
            win = torch.where(torch.isfinite(best[1]), best[0], torch.full_like(best[0], -1))
            fw = faces[win.clamp_min(0)]                                 # [H,W,3]
            wa, wb = best[3], best[4]
            wc = (1.0 - wa) - wb
            z1 = best[1]
            zf = z1.nan_to_num(posinf=1.0)
            za, zb, zc_ = pr[fw[..., 0], 2], pr[fw[..., 1], 2], pr[fw[..., 2], 2]
            ua, ub, uc = wa / za * zf, wb / zb * zf, wc / zc_ * zf
            ca, cb, cc = colors[s][fw[..., 0]], colors[s][fw[..., 1]], colors[s][fw[..., 2]]
            col = (ua[..., None] * ca + ub[..., None] * cb) + uc[..., None] * cc
            pa, pb, pc = verts[s][fw[..., 0]], verts[s][fw[..., 1]], verts[s][fw[..., 2]]
            n = torch.cross(pb - pa, pc - pa, dim=-1)
            ray = (fwd[None, None, :] + px[None, :, None] * right[None, None, :]) + py[:, None, None] * up[None, None, :]
            nn = torch.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).clamp_min(1e-20)
            rn = torch.sqrt((ray[..., 0] * ray[..., 0] + ray[..., 1] * ray[..., 1]) + ray[..., 2] * ray[..., 2])
            cosv = (((n[..., 0] * ray[..., 0] + n[..., 1] * ray[..., 1]) + n[..., 2] * ray[..., 2]) / (nn * rn)).abs()
            shaded = col if ambient == 1.0 else col * (ambient + (1.0 - ambient) * cosv)[..., None]
            color = torch.where((win >= 0)[..., None], shaded, bg.expand(H, W, 3))
            for key, val in zip(('winner', 'depth', 'runner', 'margin', 'runner_margin', 'color', 'base', 'cos'),
                                (win, z1, second[0], best[2], second[1], color, col, cosv)):
                out[key].append(val)
    return _finish(out, S, V, bg)
