"""The specification the device's line ray tracer is held to: emission_line_map (mol_transfer.f90:484-687), intensite_pixel_mol
(:691-847), integ_ray_mol (optical_depth.f90:419-599), local_line_profile (:863-927), phiProf (molecular_emission.f90:183-207)
and v_proj (:675-775), restated in numpy over the ORACLE'S OWN operators -- Oracle.move_to_grid / move_to_grid_voronoi,
cross_cell / cross_voronoi and test_exit_grid (oracle/binding.py).  No geometry of its own: the only grid test written out is
test_exit_grid_Voronoi, `icell < 0` (Voronoi.f90:1446); intersect_stars (stars.f90:812-884) is written out below.

All rays of a view are held in arrays and the live ones advance one cell per iteration (tests/column_walk.py).  The geometry
of a ray does not depend on the molecule, so a view is walked ONCE (`walk_paths`) and the cubes of every variant are formed
from the recorded steps in the order of the walk (`cube_from_paths`), in double, the results default reals.

The departures of include/mcgpu.h (mcgpu_line_map) are the specification's too: no CMB term, no ldouble_RT, no lorigine, no
stars' maps, method 1 from the sample points themselves and summed in the loop order of :616-628 into a default real."""
import numpy as np

PC_TO_AU = 648000.0 / np.pi
TINY_REAL = float(np.finfo(np.float32).tiny)
TINY_DP = float(np.finfo(np.float64).tiny)
N_RAD_RT, N_PHI_RT = 100, 36
N_VPOINTS_MAX = 200


def rotation_3d(axis, angle_deg, v):
    """utils.f90:1545-1589"""
    axis, v = np.asarray(axis, float), np.asarray(v, float)
    vp = np.dot(v, axis) * axis
    vn = v - vp
    norm = np.sqrt(np.dot(vn, vn))
    if norm < TINY_DP:
        return vp
    vn = vn / norm
    vn2 = np.cross(axis, vn)
    a = angle_deg * (np.pi / 180.0)
    return vp + norm * (np.cos(a) * vn + np.sin(a) * vn2)


def image_plane(m, q, ang_disque):
    """uvw, x_plan_image, y_plan_image of observer q = ibin + RT_n_incl * iaz (0-based) (:513-562)."""
    rt = m.rt
    ni = rt["RT_n_incl"]
    uvw = np.array([np.asarray(rt["tab_u_rt"], float).reshape(-1)[q], np.asarray(rt["tab_v_rt"], float).reshape(-1)[q],
                    np.asarray(rt["tab_w_rt"], float).reshape(-1)[q % ni]])
    az = float(np.asarray(rt["tab_RT_az"], np.float32).reshape(-1)[q // ni]) * (np.pi / 180.0)
    x = np.array([np.cos(az), np.sin(az), 0.0])
    xpi = rotation_3d(uvw, ang_disque, x) if abs(ang_disque) > TINY_REAL else x
    ypi = -np.cross(xpi, uvw)
    return uvw, xpi, ypi


def ray_starts(m, method=2, npix_x=1, npix_y=1, map_size=None, zoom=1.0, ang_disque=0.0, l_sym_ima=False):
    """The rays of a view: dict(pos [n, 3], dirn [n, 3] (the direction of propagation, away from the observer), pixelsize [n],
    q [n], ipix [n] (place in the (npix_x, npix_y) image, column-major), shape)."""
    rt = m.rt
    nRT = rt["RT_n_incl"] * rt["RT_n_az"]
    Rmax, Rmin = float(m.cfg.rout), float(m.cfg.rin)
    pos, dirn, size, qs, ipix = [], [], [], [], []
    for q in range(nRT):
        uvw, xpi, ypi = image_plane(m, q, ang_disque)
        center = uvw * (10.0 * Rmax)
        if method == 2:
            taille_pix = (map_size / zoom) / float(max(npix_x, npix_y))
            dx, dy = xpi * taille_pix, ypi * taille_pix
            Icorner = center - (0.5 * map_size) * (xpi + ypi)
            i_max = npix_x // 2 + npix_x % 2 if l_sym_ima else npix_x
            for j in range(1, npix_y + 1):
                for i in range(1, i_max + 1):
                    corner = Icorner + (i - 1) * dx + (j - 1) * dy
                    pos.append(corner + 0.5 * dx + 0.5 * dy)
                    dirn.append(-uvw); size.append(taille_pix); qs.append(q); ipix.append((i - 1) + npix_x * (j - 1))
        else:
            rmin_RT = max(uvw[2] * 0.9, 0.05) * Rmin
            rmax_RT = 2.0 * Rmax
            fact_r = np.exp((1.0 / (float(N_RAD_RT) - 1.0)) * np.log(rmax_RT / rmin_RT))
            fact_A = np.sqrt(np.pi * (fact_r - 1.0 / fact_r) / N_PHI_RT)
            cst_phi = (np.pi if l_sym_ima else 2.0 * np.pi) / float(N_PHI_RT)
            r = rmin_RT
            for ri in range(1, N_RAD_RT + 1):
                if ri > 1:
                    r = r * fact_r
                for ph in range(1, N_PHI_RT + 1):
                    phi = cst_phi * (float(ph) - 0.5)
                    pos.append(center + r * np.sin(phi) * xpi + r * np.cos(phi) * ypi)
                    dirn.append(-uvw); size.append(fact_A * r); qs.append(q); ipix.append(0)
    return dict(pos=np.array(pos), dirn=np.array(dirn), pixelsize=np.array(size), q=np.array(qs), ipix=np.array(ipix),
                method=method, npix=(npix_x, npix_y) if method == 2 else (1, 1), nRT=nRT)


def intersect_stars(m, x, y, z, u, v, w):
    """(stars.f90:812-884) icell_star per ray, 0: no star on the way."""
    stars = np.asarray(m.stars, float).reshape(-1, 6)
    d_to_star = np.full(x.shape, np.finfo(float).max)
    icell = np.zeros(x.shape, np.int64)
    for s in stars:
        dx, dy, dz = x - s[0], y - s[1], z - s[2]
        b = dx * u + dy * v + dz * w
        c = dx * dx + dy * dy + dz * dz - s[3] * s[3]
        delta = b * b - c
        ok = delta >= 0.0
        rac = np.sqrt(np.where(ok, delta, 0.0))
        s1, s2 = -b - rac, -b + rac
        inside = ok & (s1 < 0) & (s2 > 0)
        ahead = ok & ~(s1 < 0) & (s1 < d_to_star)
        d_to_star = np.where(inside, 0.0, np.where(ahead, s1, d_to_star))
        icell = np.where(inside | ahead, int(s[4]), icell)
    return icell


def walk_paths(o, m, rays, max_steps=100000):
    """Moves the rays to the grid and walks them to its edge or to the star's cell (integ_ray_mol's loop, :480-503): a list of
    (ray indices, icell, p0 [k, 3], p1 [k, 3], l_void_before, l_contrib) per iteration, real cells only."""
    voro = m.grid.get("grid_type", 1) == 3
    n_cells = m.n_cells
    p, d = rays["pos"], rays["dirn"]
    u, v, w = d[:, 0].copy(), d[:, 1].copy(), d[:, 2].copy()
    if voro:
        x, y, z, cell, hit = o.move_to_grid_voronoi(p[:, 0], p[:, 1], p[:, 2], u, v, w)
    else:
        x, y, z, cell, hit = o.move_to_grid(p[:, 0], p[:, 1], p[:, 2], u, v, w)
    live = np.asarray(hit).astype(bool)
    star = intersect_stars(m, x, y, z, u, v, w)
    nxt = np.asarray(cell, np.int32).copy()
    steps = []
    n_steps = np.zeros(len(x), np.int64)
    for _ in range(max_steps):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        c = nxt[idx]
        out = (c < 0) if voro else o.test_exit_grid(c, x[idx], y[idx], z[idx]).astype(bool)
        out = out | ((star[idx] > 0) & (c == star[idx]))
        live[idx[out]] = False
        idx, c = idx[~out], c[~out]
        if idx.size == 0:
            break
        n_steps[idx] += 1
        if voro:
            r = o.cross_voronoi(x[idx], y[idx], z[idx], u[idx], v[idx], w[idx], c, np.zeros_like(c))   # previous_cell = 0 (:502)
            x1, y1, z1, nc, lc, lv = r["x1"], r["y1"], r["z1"], r["next_cell"], r["l_contrib"], r["l_void_before"]
        else:
            x1, y1, z1, nc, lc = o.cross_cell(x[idx], y[idx], z[idx], u[idx], v[idx], w[idx], c)
            lv = np.zeros_like(lc)
        real = c <= n_cells
        k = idx[real]
        steps.append((k, c[real].astype(np.int64), np.stack([x[k], y[k], z[k]], 1),
                      np.stack([x1[real], y1[real], z1[real]], 1), np.asarray(lv, float)[real], np.asarray(lc, float)[real]))
        x[idx], y[idx], z[idx], nxt[idx] = x1, y1, z1, nc
    return dict(steps=steps, n_rays=len(x), hit=np.asarray(hit).astype(bool), n_steps=n_steps, unfinished=int(live.sum()),
                dirn=d)


def v_proj(m, mol, ic, p, d):
    """(molecular_emission.f90:675-775) for cells ic (0-based) at points p [k, 3] along d [k, 3]."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    u, v, w = d[:, 0], d[:, 1], d[:, 2]
    n = m.n_cells
    if m.grid.get("grid_type", 1) == 3:
        vx = np.asarray(mol["vxyz"], float).reshape(n, 3)[ic]
        return vx[:, 0] * u + vx[:, 1] * v + vx[:, 2] * w
    l3d = bool(m.grid["l3D"])
    if int(mol.get("vfield_mode", 1)) == 2:
        vf = np.asarray(mol["vfield"], np.float32).reshape(3, n).astype(float)
        a1, a2, a3 = vf[0][ic], vf[1][ic], vf[2][ic]
        coord = int(mol["vfield_coord"])
        flip = (z < 0) if not l3d else np.zeros(z.shape, bool)
        if coord == 1:
            vx, vy, vz = a1, a2, a3
        elif coord == 2:
            phi = np.arctan2(y, x)
            vx = np.cos(phi) * a1 - np.sin(phi) * a2
            vy = np.sin(phi) * a1 + np.cos(phi) * a2
            vz = np.where(flip, -a3, a3)
        else:
            vt = np.where(flip, -a3, a3)
            rcyl2 = x * x + y * y
            r2 = rcyl2 + z * z
            rcyl, r = np.sqrt(rcyl2), np.sqrt(r2)
            ct, st = rcyl / r, z / r
            cp, sp = x / rcyl, y / rcyl
            vz = -vt * ct + a1 * st
            vr = vt * st + a1 * ct
            vx = vr * cp - a2 * sp
            vy = vr * sp + a2 * cp
        return vx * u + vy * v + vz * w
    vel = np.asarray(mol["vfield"], np.float32).astype(float)[ic]
    chi = float(np.float32(mol.get("chi_infall", 1.0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        if mol.get("lkeplerian"):
            r = np.sqrt(x * x + y * y)
            ok = r > TINY_DP
            norm = 1.0 / np.where(ok, r, 1.0)
            vx, vy = -y * norm * vel, x * norm * vel
            if mol.get("linfall"):
                r3 = np.sqrt(x * x + y * y + z * z)
                norm = 1.0 / np.where(ok, r3, 1.0)
                vx = vx - chi * x * norm * vel
                vy = vy - chi * y * norm * vel
                vz = 0.0 - chi * z * norm * vel
                return np.where(ok, vx * u + vy * v + vz * w, 0.0)
            return np.where(ok, vx * u + vy * v, 0.0)
        r = np.sqrt(x * x + y * y + z * z)
        ok = r > TINY_DP
        norm = 1.0 / np.where(ok, r, 1.0)
        return np.where(ok, (x * norm * vel) * u + (y * norm * vel) * v + (z * norm * vel) * w, 0.0)


def cube_from_paths(m, mol, rays, paths, lonly_top=False, lonly_bottom=False, raw=False):
    """dict(spectrum [nRT, nTrans, n_speed, npix_y, npix_x] float32, continu [nRT, nTrans, npy, npx] float32, I0, I0c (double,
    per ray, before the units), hist (histogram of n_vpoints, index = value), half_dist (the smallest distance of
    dv / dv_line * 20 from a half-integer over the steps where the rounding decides, 1 <= q <= 201), longest)."""
    voro = m.grid.get("grid_type", 1) == 3
    n = m.n_cells
    ts = np.asarray(mol["tab_speed"], float)
    fr = np.asarray(mol["transfreq"], float)
    nT, ns = fr.size, ts.size
    kmol = np.asarray(mol["kappa_mol_o_freq"], float).reshape(nT, n)
    emol = np.asarray(mol["emissivite_mol_o_freq"], float).reshape(nT, n)
    edust = np.asarray(mol["emissivite_dust"], float).reshape(nT, n)
    kabs = np.asarray(mol["kappa_abs_LTE"], float).reshape(nT, -1)
    vd = getattr(m, "variable_dust", None)
    cls = np.zeros(n, np.int64) if vd is None else np.asarray(vd["p_icell"], np.int64) - 1
    kf = np.asarray(m.kappa_factor, float)
    norme, s2 = np.asarray(mol["norme_phiProf_m1"], float), np.asarray(mol["sigma2_phiProf_m1"], float)
    nr = paths["n_rays"]
    d_all = paths["dirn"]
    tau, I0 = np.zeros((nr, nT, ns)), np.zeros((nr, nT, ns))
    tau_c, I0c = np.zeros((nr, nT)), np.zeros((nr, nT))
    hist = np.zeros(N_VPOINTS_MAX + 1, np.int64)
    half = np.inf
    for idx, c, p0, p1, lv, lc in paths["steps"]:
        if idx.size == 0:
            continue
        ic = c - 1
        d = d_all[idx]
        v0 = v_proj(m, mol, ic, p0, d)
        if voro:
            n_vp = np.ones(idx.size, np.int64)
            vel = v0[:, None]
        else:
            v1 = v_proj(m, mol, ic, p1, d)
            dv = np.abs(v1 - v0).astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                qf = (dv / np.asarray(mol["dv_line"], np.float32)[ic]) * np.float32(20.0)        # single precision
            q = qf.astype(float)
            decides = (q >= 1.0) & (q <= N_VPOINTS_MAX + 1.0)
            if decides.any():
                half = min(half, float(np.min(np.abs(q[decides] - np.floor(q[decides]) - 0.5))))
            nint = np.floor(np.where(np.isfinite(q), np.minimum(q, 1e6), 1e6) + 0.5).astype(np.int64)   # half away from zero (q >= 0)
            n_vp = np.minimum(np.maximum(2, nint), N_VPOINTS_MAX)
            vel = np.zeros((idx.size, int(n_vp.max())))
            for ivp in range(2, int(n_vp.max())):
                on = ivp <= n_vp - 1
                delta = lv[on] + (float(ivp) / n_vp[on].astype(float)) * lc[on]
                vel[on, ivp - 1] = v_proj(m, mol, ic[on], p0[on] + delta[:, None] * d[on], d[on])
            vel[:, 0] = v0
            vel[np.arange(idx.size), n_vp - 1] = v1
        hist += np.bincount(n_vp, minlength=N_VPOINTS_MAX + 1)
        P = np.zeros((idx.size, ns))
        for ivp in range(int(n_vp.max())):
            on = ivp < n_vp
            t = ts[None, :] - vel[on, ivp][:, None]
            P[on] = P[on] + norme[ic[on]][:, None] * np.exp(-s2[ic[on]][:, None] * t ** 2)
        P = P / n_vp.astype(float)[:, None]
        ft = np.ones(idx.size)
        if lonly_top:
            ft[p0[:, 2] < 0.0] = 0.0
        if lonly_bottom:
            ft[p0[:, 2] > 0.0] = 0.0
        for i in range(nT):
            kappa_cont = kabs[i][cls[ic]] * kf[ic]
            opacity = kmol[i][ic][:, None] * P * ft[:, None] + kappa_cont[:, None]
            dtau = lc[:, None] * opacity
            dtau_c = lc * kappa_cont
            Snu = (emol[i][ic][:, None] * P * ft[:, None] + edust[i][ic][:, None]) / (opacity + 1.0e-300)
            Snu_c = edust[i][ic] / (kappa_cont + 1.0e-300)
            I0[idx, i] = I0[idx, i] + np.exp(-tau[idx, i]) * (1.0 - np.exp(-dtau)) * Snu
            I0c[idx, i] = I0c[idx, i] + np.exp(-tau_c[idx, i]) * (1.0 - np.exp(-dtau_c)) * Snu_c
            tau[idx, i] = tau[idx, i] + dtau
            tau_c[idx, i] = tau_c[idx, i] + dtau_c
    dist = float(m.cfg.distance)
    sr = (rays["pixelsize"] / (dist * PC_TO_AU)) ** 2
    IP = I0 * sr[:, None, None] * fr[None, :, None]
    IPc = I0c * sr[:, None] * fr[None, :]
    npx, npy = rays["npix"]
    nRT = rays["nRT"]
    spec = np.zeros((nRT, nT, ns, npy * npx), np.float32)
    cont = np.zeros((nRT, nT, npy * npx), np.float32)
    if rays["method"] == 2:
        spec[rays["q"], :, :, rays["ipix"]] = IP.astype(np.float32)
        cont[rays["q"], :, rays["ipix"]] = IPc.astype(np.float32)
    else:
        for r in range(nr):                      # the loop order of :616-628, `spectrum = spectrum + IP` in a default real
            q = rays["q"][r]
            spec[q, :, :, 0] = (spec[q, :, :, 0].astype(float) + IP[r]).astype(np.float32)
            cont[q, :, 0] = (cont[q, :, 0].astype(float) + IPc[r]).astype(np.float32)
    out = dict(spectrum=spec.reshape(nRT, nT, ns, npy, npx), continu=cont.reshape(nRT, nT, npy, npx), hist=hist, half_dist=half,
               longest=int(paths["n_steps"].max()) if nr else 0)
    if raw:
        out.update(I0=I0, I0c=I0c, tau=tau, tau_c=tau_c)
    return out
