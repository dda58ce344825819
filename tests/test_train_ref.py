"""tests/train_ref.py on the CPU: every frame the GPU tests use is off the rate floor and well
conditioned (the float32 oracle within 2^-16 of its own float64 run), the restated unit counts
and workgroup arithmetic give what the GPU cases rely on, and the float64 Adam agrees with
train_oracle.Adam."""
import math

import numpy as np
import pytest
import torch

import train_ref as R

OWN_FRAMES = [c for c in R.CASES if c.frames_of == c.name]


@pytest.mark.parametrize("case", OWN_FRAMES, ids=lambda c: c.name)
def test_frames_are_off_the_floor_and_well_conditioned(case):
    for d, f in enumerate(R.case_frames(case)):
        what = f"{case.name} frame {d} (seed {R.case_seed(case, d)})"
        assert f.e32 <= R.E32_MAX, (what, f.e32)
        assert f.p_min >= R.P_MIN, (what, f.p_min)
        assert -4.6 + 1 <= f.ls_lo and f.ls_hi <= 5 - 1, (what, f.ls_lo, f.ls_hi)
        assert min(f.S) > 0, (what, f.S)
        assert len(f.g64) == len(f.sizes) and sum(f.sizes) == f.N + f.P
        u = R.units(case.H, case.W, **case.arch)
        assert (u.N, u.P) == (f.N, f.P)
        # the float64 oracle is the float32 oracle's reference for the loss row too
        for a, b, tol in zip(f.row32, f.row64, (1e-6, 1e-6, 1e-6)):
            assert abs(a - b) <= tol * abs(b), (what, a, b)
        assert all(math.isfinite(x) for x in f.eval64)


def test_default_setting_gives_the_same_frame_bit_for_bit():
    """frame()'s quantiser setting defaults to the warm-up's: a call that spells the defaults out
    gives the cached frame's inputs and float64 gradients bit for bit (the same generator calls in
    the same order)."""
    c = R.CASE["hop"]
    f = R.case_frames(c)[1]
    g = R.frame(c.H, c.W, R.case_seed(c, 1), c.yuv420, qtype="softround", ntype="kumaraswamy", T=R.TEMP, nparam=R.NOISE_A,
                lat_plant=None, **c.arch)
    assert g is not f
    for k in ("lat", "params", "target", "noise"):
        assert torch.equal(getattr(f, k), getattr(g, k)), k
    assert f.row64 == g.row64 and f.row32 == g.row32 and f.eval64 == g.eval64
    assert len(f.g64) == len(g.g64) and all(np.array_equal(a, b) for a, b in zip(f.g64, g.g64))
    assert all(np.array_equal(a, b) for a, b in zip(f.g32, g.g32))
    assert (f.e32, f.p_min, f.S) == (g.e32, g.p_min, g.S)
    # 0.05 randn, as before the plant existed
    gen = torch.Generator().manual_seed(1000 + R.case_seed(c, 1))
    lat = torch.cat([(0.05 * torch.randn(h, w, generator=gen)).reshape(-1) for h, w in f.mp.sizes])
    assert torch.equal(lat, f.lat)


SCHEDULE_FRAMES = [(s, c) for s in R.SCHEDULE + [R.STE_END] for c in R.SCHEDULE_CASES]


@pytest.mark.parametrize("setting,case", SCHEDULE_FRAMES, ids=lambda x: x if isinstance(x, str) else x.name)
def test_schedule_frames_are_off_the_floor_and_well_conditioned(setting, case):
    c = R.CASE[case]
    frs = R.schedule_frames(setting, case)
    assert len(frs) == R.SCHEDULE_D
    e = [f.e32 for f in frs]
    print(f"\n{setting.name} {case}: e32 2^{math.log2(min(e)):.1f} .. 2^{math.log2(max(e)):.1f}, "
          f"p_min {min(f.p_min for f in frs):.1e}")
    for d, f in enumerate(frs):
        what = f"{setting.name} {case} frame {d} (seed {R.schedule_seed(setting, case, d)})"
        assert f.e32 <= R.E32_MAX, (what, f.e32)
        assert f.p_min >= R.P_MIN, (what, f.p_min)
        assert -4.6 + 1 <= f.ls_lo and f.ls_hi <= 5 - 1, (what, f.ls_lo, f.ls_hi)
        assert (f.N, f.P) == (R.units(c.H, c.W, **c.arch).N, R.units(c.H, c.W, **c.arch).P)
        if setting.name == "hardround":
            # dq = 0: the latent gradients are exactly zero, and nothing else is
            assert all(not f.g64[i].any() and f.S[i] == 0 for i in range(f.n_grids))
            assert min(f.S[f.n_grids:]) > 0, (what, f.S)
            assert not f.noise.any()
        else:
            assert min(f.S) > 0, (what, f.S)
        for a, b in zip(f.row32, f.row64):
            assert abs(a - b) <= 1e-6 * abs(b), (what, a, b)
        assert (setting.ntype == "none") == (not f.noise.any())
        if setting.ntype == "gaussian":
            assert 0.9 * setting.nparam < float(f.noise.std()) < 1.1 * setting.nparam
        x = f.lat * f.gain
        if setting.lat_plant == "coarse":
            assert bool(torch.round(x[-f.sizes[f.n_grids - 1]:]).any())
        if setting.lat_plant == "half":
            # on the peak of ste's derivative at T = 1e-4: |frac - 1/2| <= 8.5e-4 everywhere
            fr = (x.double() - torch.floor(x.double()) - 0.5).abs()
            assert float(fr.max()) <= 8.5e-4 and float(fr.min()) == 0


def test_schedule_table():
    assert [s.name for s in R.SCHEDULE] == ["warmup-a1", "main-start", "main-mid", "main-end", "ste-warm", "true-ste",
                                            "alone-end", "noise-only", "hardround"]
    m = R.SETTING
    assert (m["main-start"].T, m["main-start"].nparam) == (0.3, 0.25)
    assert (m["main-mid"].T, m["main-mid"].nparam) == (0.2, 0.175)
    assert (m["main-end"].T, m["main-end"].nparam) == (0.1, 0.1)
    assert (m["warmup-a1"].qtype, m["warmup-a1"].ntype, m["warmup-a1"].nparam) == ("softround", "kumaraswamy", 1.0)
    assert (R.STE_END.T, R.STE_END.qtype) == (1e-4, "true_ste")
    # the preset's own figures (ccmi/train.py)
    from ccmi import train as T
    main = [p for p in T.C3X_PHASES if p.quantizer_type == "softround"]
    assert {p.softround_temperature for p in main} == {(0.3, 0.1)} and {p.noise_parameter for p in main} == {(0.25, 0.1)}
    ste = [p for p in T.C3X_PHASES if p.quantizer_type == "ste"]
    assert ste and all(p.softround_temperature == (1e-4, 1e-4) for p in ste)
    # seeds: distinct among themselves and from every case's
    seeds = [R.schedule_seed(s, c, d) for s, c in SCHEDULE_FRAMES if s.name != "hardround" for d in range(R.SCHEDULE_D)]
    older = [R.case_seed(c, d) for c in OWN_FRAMES for d in range(c.D)]
    assert len(set(seeds + older)) == len(seeds) + len(older)
    for (name, case, d) in R.SCHEDULE_RESEED:
        assert (name in R.SETTING or name == R.STE_END.name) and case in R.SCHEDULE_CASES and d < R.SCHEDULE_D
    # hardround's frames are true-ste's, latent gradients zeroed
    a, b = R.schedule_frames("hardround", "hop")[0], R.schedule_frames("true-ste", "hop")[0]
    assert a.row64 == b.row64 and all(np.array_equal(x, y) for x, y in zip(a.g64[a.n_grids:], b.g64[b.n_grids:]))


def test_cases_share_or_own_their_frames():
    for c in R.CASES:
        o = R.CASE[c.frames_of]
        assert (o.H, o.W, o.D, o.yuv420, o.arch) == (c.H, c.W, c.D, c.yuv420, c.arch)
    seeds = [R.case_seed(c, d) for c in OWN_FRAMES for d in range(c.D)]
    assert len(set(seeds)) == len(seeds)
    for (name, d) in R.RESEED:
        assert name in R.CASE and d < R.CASE[name].D


def test_unit_counts():
    u = R.units(33, 65)
    assert (u.arm, u.sp, u.head, u.head_regs) == (31, 6, 17, 34)
    u = R.units(81, 129)
    assert (u.arm, u.sp, u.head) == (98, 18, 82)
    u = R.units(300, 450)
    assert (u.arm, u.sp, u.head, u.N) == (810, 152, 1055, 180132)
    assert u.latgrad_passes == 2 and u.loss_passes == 2     # 300 x 450 = 135,000 pixels, N + P = 181,457
    assert R.units(128, 192).latgrad_passes == 1            # the largest older gradient test: one pass
    assert R.SUM_PASS == 131072


def test_workgroup_arithmetic_at_256_cus():
    cus = 256
    assert R.max_workgroups_per_frame(cus, 2048, 256) == 1
    assert R.max_workgroups_per_frame(cus, 2048, 128) == 2
    assert R.max_workgroups_per_frame(cus, 128, 256) == 16
    assert R.max_workgroups_per_frame(cus, 128, 128) == 32
    assert R.max_workgroups_per_frame(cus, 1, 256) == 2048
    for c in R.CASES:
        it = R.case_iterations(c, cus)
        B = R.batch_of(c, cus)
        u = R.units(c.H, c.W, **c.arch)
        if c.group == "a":
            # one workgroup per frame (two for the 128-thread head): every loop at least 3 times
            assert B == 2048 and all(v >= 3 for v in it.values()), (c.name, it)
            assert it["arm"] == u.arm
        elif c.group == "b":
            # 2 ARM workgroups; at most 16 for the 18 3x3 tiles and 32 for the 82 chunks, neither a
            # divisor: some workgroups run one iteration more than others
            assert B == 128 and cus // B == 2 and it["arm"] == 49
            assert it["sp"] >= 2 and u.sp % R.max_workgroups_per_frame(cus, B, 256) != 0
            assert it["head"] >= 3 and u.head % R.max_workgroups_per_frame(cus, B, 128) != 0
        else:
            assert B == 1 and it["arm"] == 4 and u.arm % cus != 0    # 810 tiles on 256 workgroups: 4 or 3 each
            assert u.latgrad_passes == 2 and u.loss_passes == 2
    assert R.case_iterations(R.CASE["hop"], cus) == {"arm": 31, "sp": 6, "head": 9}
    assert R.case_iterations(R.CASE["hop-head-regs"], cus)["head"] == 34


def test_norm_rounding_count():
    # 33 x 65 hop: 4,252 entries on 5 workgroups, one pass; 300 x 450: 128 workgroups, two passes
    assert R.sumsq_roundings(4252) == (4 + 6 + 3 + 5) / 2 + 1
    assert R.sumsq_roundings(181457) == (8 + 6 + 3 + 128) / 2 + 1


def test_adam64_against_the_oracle_adam():
    """Two clipped steps of train_oracle.Adam (torch float32) against adam64 step by step from the
    oracle's own state.  torch multiplies by the doubles 1 - 0.9 and 1 - 0.999 rounded to float, the
    kernel (and adam64) by 1.f - 0.9f = 0.10000002 and 1.f - 0.999f = 0.00099998713: 4 and 216
    roundings (2^-24) apart, on top of the 3 and 5 of the float32 evaluation, so m' is held to 8 on
    T_m, v' to 224, and the step to 8 on the m' term and 120 on |s| (224 / 2 under the square root,
    and adam_bounds' own 8).  A wrong bias correction, clip coefficient or epsilon placement is
    thousands of times that."""
    import train_oracle as to
    c = R.CASE["hop"]
    f = R.case_frames(c)[1]
    st = to.TrainState(f.mp, f.lat_grids)
    assert torch.equal(torch.cat([x.detach().reshape(-1) for x in st.params()[f.n_grids:]]), f.params)
    target = f.target_t
    opt = to.Adam(st.params(), 1e-2)
    flat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs]).numpy().copy()
    for t in (1, 2):
        to.grads(st, target, "softround", R.TEMP, R.LMBDA, False, noise=f.noise)
        G, m0, v0, p0 = flat([p.grad for p in st.params()]), flat(opt.m), flat(opt.v), flat(st.params())
        if t == 1:
            # the frame's own step (its float32 run used one thread, this one the default: the
            # bits differ, the gradient does not)
            tol = np.repeat([4 * R.E32_MAX * s for s in f.S], f.sizes)
            assert np.all(np.abs(G.astype(np.float64) - np.concatenate(f.g64)) <= tol)
        norm = np.float32(math.sqrt(float((G.astype(np.float64) ** 2).sum())))
        assert norm > 0.1                 # the clip is active
        opt.step(clip=0.1)
        r = R.adam64(G, m0, v0, p0, norm, 0.1, 1e-2, t)
        k3, k8 = R._k(3), R._k(8)
        tm = 8 / 3 * k3 * r.T_m
        tv = 224 * R.E * r.v * 1.001
        tp = 8 / 3 * k3 * r.lr_bc1 * r.T_m / r.d + (224 / 2 + 8) / 8 * k8 * np.abs(r.s) + R.E * np.abs(r.p)
        for name, got, ref, tol in (("m", flat(opt.m), r.m, tm), ("v", flat(opt.v), r.v, tv), ("p", flat(st.params()), r.p, tp)):
            err = np.abs(got - ref)
            assert np.all(err <= tol + 1e-45), (t, name, float((err / (tol + 1e-45)).max()))
