"""GPU: the error-map kernels (csrc/error_map.hip) ARE the numpy model of tests/error_map_cases.py -- the race keys to the accuracy of
logf and one division, the selection from the device's own keys / the refinement to pixels / the EMA update bit for bit -- and the Python
surface on top (nerf/utils.get_rays(seed=), ErrorMaps, GraphedTrainStep.image) hands the same bits on.  That the model draws the stated
distribution is tests/test_error_map_cases.py's business (CPU)."""

import numpy as np
import pytest
import torch

import error_map_cases as em
import oracle
import synthetic_scene as sc

pytestmark = pytest.mark.gpu

KEY_RTOL = 8 * 2.0 ** -24   # logf <= 1 ulp (ROCm math tables), one correctly rounded division, margin
FRAMES = [(800, 800), (37, 101), (1, 1)]
MAPS = ['ones', 'uniform', 'loguniform', 'mixed']


def _map(kind, B, cells, rng):
    if kind == 'ones':
        return np.ones((B, cells), np.float32)
    if kind == 'uniform':
        return rng.uniform(0.01, 1.0, (B, cells)).astype(np.float32)
    if kind == 'loguniform':
        return np.exp(rng.uniform(np.log(1e-12), np.log(1e6), (B, cells))).astype(np.float32)
    w = rng.uniform(0.01, 1.0, (B, cells)).astype(np.float32)   # zeros, negatives, NaN, inf and subnormals sprinkled in: > 1/3 undrawable
    i = np.arange(cells)
    w[:, i % 5 == 0] = 0.0
    w[:, i % 7 == 2] = -0.5
    w[:, i % 11 == 3] = np.nan
    w[:, i % 13 == 4] = np.inf
    w[:, i % 17 == 5] = 1e-42
    w[:, i % 19 == 6] = -np.inf
    return w


def _draw(w_t, res, N, H, W, seed, seed_dev=None, extras=True):
    """one ngp_error_map_draw call -> numpy (inds, coarse, keys, n_drawable)"""
    import _ngp_capi as capi
    B, cells = w_t.shape
    dev = w_t.device
    inds = torch.full((B, N), -7, dtype=torch.int64, device=dev)
    coarse = torch.full((B, N), -7, dtype=torch.int64, device=dev)
    keys = torch.full((B, cells), -1.0, dtype=torch.float32, device=dev) if extras else None
    nd = torch.full((B,), -1, dtype=torch.int32, device=dev) if extras else None
    capi.check(capi.lib.ngp_error_map_draw(w_t.data_ptr(), B, res, N, H, W, seed, capi.ptr(seed_dev), inds.data_ptr(), coarse.data_ptr(),
                                           capi.ptr(keys), capi.ptr(nd), capi.stream()))
    torch.cuda.synchronize()
    return (inds.cpu().numpy(), coarse.cpu().numpy(), None if keys is None else keys.cpu().numpy(), None if nd is None else nd.cpu().numpy())


@pytest.mark.parametrize('res', [1, 3, 8, 31, 32, 33, 128])
def test_draw_is_the_model(res):
    """every (N, B, map, frame) of the issue's grid at this resolution: below, at and above one wave / one 1024-lane pass"""
    dev = torch.device('cuda')
    cells = res * res
    rng = np.random.default_rng(res)
    worst, tie_break_cases, n_calls = 0.0, 0, 0
    for B in (1, 3):
        for kind in MAPS:
            w = _map(kind, B, cells, rng)
            w_t = torch.from_numpy(w).to(dev)
            seed = 1000 * res + 10 * B + MAPS.index(kind)
            ok = em.drawable(w)
            k64 = np.stack([em.keys64(w[b], b, seed) for b in range(B)])
            want_inf = ~ok | (k64 > em.FLT_MAX)
            for N in sorted({n for n in (1, cells // 4, cells - 1, cells) if 1 <= n <= cells}):
                for H, W in FRAMES:
                    inds, coarse, keys, nd = _draw(w_t, res, N, H, W, seed)
                    n_calls += 1
                    # uniforms and keys
                    assert np.array_equal(np.isposinf(keys), want_inf), (res, B, kind, N)
                    fin = ~want_inf
                    if fin.any():
                        rel = np.abs(keys[fin].astype(np.float64) - k64[fin]) / k64[fin]
                        worst = max(worst, float(rel.max()))
                        assert rel.max() <= KEY_RTOL, (res, B, kind, float(rel.max()))
                    assert np.array_equal(nd, ok.sum(1))
                    for b in range(B):
                        # selection, exact: the N smallest of the DEVICE's keys by (bits, index), ascending
                        sel = em.select(keys[b], N)
                        assert np.array_equal(coarse[b], sel), (res, B, kind, N, b)
                        assert np.all(np.diff(coarse[b]) > 0) and coarse[b].min() >= 0 and coarse[b].max() < cells
                        # refinement, exact, inside the cell's pixel range and the frame
                        assert np.array_equal(inds[b], em.refine(sel, b, seed, res, H, W)), (res, B, kind, N, H, W, b)
                        row, col = inds[b] // W, inds[b] % W
                        f = np.float32
                        for pix, cell, size in ((row, sel // res, H), (col, sel % res, W)):
                            step = np.float64(f(size) / f(res))
                            assert np.all(pix >= np.minimum(np.floor(cell * step), size - 1)) and np.all(pix <= np.minimum(np.ceil((cell + 1) * step), size - 1))
                        if N > ok[b].sum():
                            tie_break_cases += 1   # undrawable cells were needed: lowest index first (part of `sel`)
                            spare = np.setdiff1d(sel, np.nonzero(fin[b])[0])
                            undrawable = np.nonzero(want_inf[b])[0]
                            assert np.array_equal(spare, undrawable[:spare.size])
    print(f'res {res}: {n_calls} draws, largest relative key error {worst / 2.0 ** -24:.2f} x 2^-24, {tie_break_cases} tie-break cases')
    assert tie_break_cases >= 1   # the mixed map with N above its drawable count


def test_seed_host_word_device_word_and_images():
    dev = torch.device('cuda')
    res, N, H, W = 33, 200, 480, 640
    rng = np.random.default_rng(5)
    row = rng.uniform(0.01, 1.0, (1, res * res)).astype(np.float32)
    w_t = torch.from_numpy(np.repeat(row, 3, 0)).to(dev)   # three identical rows
    a = _draw(w_t, res, N, H, W, 77)
    b = _draw(w_t, res, N, H, W, 77)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                      # the same seed: the same outputs
    word = torch.tensor([77], dtype=torch.int32, device=dev)
    c = _draw(w_t, res, N, H, W, 0, seed_dev=word)
    assert all(np.array_equal(x, y) for x, y in zip(a, c))                      # seed = k, no device word == seed = 0, device word k
    word.fill_(70)
    c = _draw(w_t, res, N, H, W, 7, seed_dev=word)
    assert all(np.array_equal(x, y) for x, y in zip(a, c))                      # the two words add
    d = _draw(w_t, res, N, H, W, 78)
    assert not np.array_equal(a[1], d[1]) and not np.array_equal(a[2], d[2])    # different seeds differ
    assert not np.array_equal(a[1][0], a[1][1]) and not np.array_equal(a[1][1], a[1][2])   # identical rows, different images: different sets
    e = _draw(w_t, res, N, H, W, 77, extras=False)                              # the optional outputs are optional
    assert np.array_equal(a[0], e[0]) and np.array_equal(a[1], e[1])


@pytest.mark.parametrize('N', [1, 63, 64, 65, 4096])
def test_update_is_the_model(N):
    import _ngp_capi as capi
    dev = torch.device('cuda')
    n_cells = 128 * 128
    rng = np.random.default_rng(N)
    row = rng.uniform(0.0, 2.0, n_cells).astype(np.float32)
    coarse = np.sort(rng.permutation(n_cells)[:N]).astype(np.int64)
    img, tgt = rng.random((N, 3)).astype(np.float32), rng.random((N, 3)).astype(np.float32)
    for bad in (False, True):
        c = coarse.copy()
        if bad and N >= 63:   # out-of-range cells skip their rays and touch nothing else
            c[[0, 7, 20, 41]] = [-1, n_cells, 1 << 40, -(1 << 33)]
        elif bad:
            c[0] = n_cells
        row_t, c_t = torch.from_numpy(row).to(dev), torch.from_numpy(c).to(dev)
        img_t, tgt_t = torch.from_numpy(img).to(dev), torch.from_numpy(tgt).to(dev)
        capi.check(capi.lib.ngp_error_map_update(row_t.data_ptr(), c_t.data_ptr(), img_t.data_ptr(), tgt_t.data_ptr(), N, n_cells, 0.1, 0.9, capi.stream()))
        got = row_t.cpu().numpy()
        want = em.update(row, c, img, tgt, 0.1, 0.9)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        named = c[(c >= 0) & (c < n_cells)]
        rest = np.setdiff1d(np.arange(n_cells), named)
        assert np.array_equal(got[rest].view(np.uint32), row[rest].view(np.uint32))   # untouched cells keep their bits
        assert not np.array_equal(got[named], row[named]) or named.size == 0


def test_error_maps_object_and_get_rays_seed():
    from nerf import utils
    dev = torch.device('cuda')
    H, W, N, B = 120, 160, 300, 2
    maps = utils.ErrorMaps(5, dev)
    assert maps.maps.shape == (5, 128 * 128) and maps.maps.dtype == torch.float32 and bool((maps.maps == 1).all())
    rng = np.random.default_rng(1)
    maps.maps.copy_(torch.from_numpy(rng.uniform(0.01, 1.0, (5, 128 * 128)).astype(np.float32)))
    poses = torch.eye(4, device=dev)[None].repeat(B, 1, 1)
    poses[:, :3, 3] = torch.tensor([[0.1, 0.2, 2.0], [-0.3, 0.0, 1.5]], device=dev)
    intr = (150.0, 140.0, 80.0, 60.0)
    emap = maps.maps[1:3]
    # seed=: the native draw, then the rays kernel as on the torch path (the same bits for the same pixels)
    out = utils.get_rays(poses, intr, H, W, N, error_map=emap, seed=9)
    inds, coarse = utils.draw_error_map(emap, H, W, N, 9)
    assert torch.equal(out['inds'], inds) and torch.equal(out['inds_coarse'], coarse) and out['inds'].shape == (B, N)
    for b in range(B):
        sel = em.select(np.float32(em.keys64(emap[b].cpu().numpy(), b, 9)), N)
        assert np.intersect1d(sel, coarse[b].cpu().numpy()).size >= N - 2   # (fp32 vs fp64 keys may swap a pair at the threshold)
    ro, rd = utils.pose_rays(poses, intr, H, W, inds)
    assert torch.equal(out['rays_o'], ro) and torch.equal(out['rays_d'], rd)
    step = torch.tensor([9], dtype=torch.int32, device=dev)
    bufs = (torch.empty(B, N, 3, device=dev), torch.empty(B, N, 3, device=dev))
    out2 = utils.get_rays(poses, intr, H, W, N, error_map=emap, seed=step, out=bufs)
    assert torch.equal(out2['inds'], inds) and torch.equal(bufs[0].view(B, N, 3), ro) and torch.equal(bufs[1].view(B, N, 3), rd)
    one = maps.draw(1, H, W, N, 9)
    assert torch.equal(one[0], inds[:1]) and torch.equal(one[1], coarse[:1])
    # patch_size > 1 keeps ignoring the map (and the seed)
    patch = utils.get_rays(poses, intr, H, W, 64, error_map=emap, patch_size=4, seed=9)
    assert 'inds_coarse' not in patch
    # seed=None: today's torch path, the old helpers called directly
    torch.manual_seed(3)
    old = utils.get_rays(poses, intr, H, W, N, error_map=emap)
    torch.manual_seed(3)
    t_inds, t_coarse = utils._draw_pixels(B, H, W, N, emap, 1, dev)
    assert torch.equal(old['inds'], t_inds) and torch.equal(old['inds_coarse'], t_coarse)
    ro, rd = utils.pose_rays(poses, intr, H, W, t_inds)
    assert torch.equal(old['rays_o'], ro) and torch.equal(old['rays_d'], rd)
    # update: in place on the row, the model's bits; the maps round-trip as a plain tensor
    img, tgt = torch.rand(N, 3, device=dev), torch.rand(N, 3, device=dev)
    before = maps.maps.clone()
    maps.update(1, coarse[0], img, tgt)
    want = em.update(before[1].cpu().numpy(), coarse[0].cpu().numpy(), img.cpu().numpy(), tgt.cpu().numpy())
    assert np.array_equal(maps.maps[1].cpu().numpy().view(np.uint32), want.view(np.uint32))
    keep = [0, 2, 3, 4]
    assert torch.equal(maps.maps[keep], before[keep])
    with pytest.raises(RuntimeError, match='float32'):
        maps.update(1, coarse[0], img.half(), tgt)
    with pytest.raises(RuntimeError, match='without replacement'):
        utils.draw_error_map(torch.ones(1, 9, device=dev), 8, 8, 10, 1, res=3)


def test_draw_and_update_replay_from_a_graph():
    """no workspace, no read-back, the seed from a device word: both launches capture, and replays with the word bumped in between are
    the eager sequence"""
    from nerf import utils
    dev = torch.device('cuda')
    res, H, W, N = 32, 100, 90, 128
    rng = np.random.default_rng(2)
    w0 = torch.from_numpy(rng.uniform(0.01, 1.0, (1, res * res)).astype(np.float32)).to(dev)
    img, tgt = torch.rand(N, 3, device=dev), torch.rand(N, 3, device=dev)

    def once(maps, word):
        inds, coarse = maps.draw(0, H, W, N, word)
        maps.update(0, coarse[0], img, tgt)
        return inds, coarse

    eager_maps, word = utils.ErrorMaps(1, dev, res=res), torch.zeros(1, dtype=torch.int32, device=dev)
    eager_maps.maps.copy_(w0)
    eager = []
    for k in range(3):
        word.fill_(40 + k)
        inds, coarse = once(eager_maps, word)
        eager.append((inds.clone(), coarse.clone(), eager_maps.maps.clone()))
    graph_maps = utils.ErrorMaps(1, dev, res=res)
    graph_maps.maps.copy_(w0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        inds, coarse = once(graph_maps, word)
    assert torch.equal(graph_maps.maps, w0)   # capturing executes nothing
    for k in range(3):
        word.fill_(40 + k)
        g.replay()
        assert torch.equal(inds, eager[k][0]) and torch.equal(coarse, eager[k][1]) and torch.equal(graph_maps.maps, eager[k][2])
    assert not torch.equal(eager[0][1], eager[1][1])


# ---- GraphedTrainStep.image ----
N_RAYS = 256
KW = dict(staged=False, bg_color=1, perturb=False, force_all_rays=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)
LOSS_RTOL = (3 * N_RAYS + 2) * 2.0 ** -24   # worst case of an fp32 sum of 3 N non-negative terms (+ the division)


def _make_ngp(dev):
    import raymarching
    from nerf.network_ff import NeRFNetwork
    from optim import NGPAdam
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    model.train()
    model.density_grid.copy_(torch.from_numpy(sc.occupancy_density()))
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    model.iter_density = 16
    return model, NGPAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)


@pytest.fixture(scope='module')
def scene():
    dev = torch.device('cuda')
    occ = torch.from_numpy(sc.occupancy_density()).to(dev)
    bits = torch.from_numpy(oracle.packbits(sc.occupancy_density(), 10.0)).to(dev)
    batches = []
    for i in range(23):
        o, d, gt = sc.training_batch(N_RAYS, seed=300 + i)
        batches.append((torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev), torch.from_numpy(gt).to(dev)))

    def keep(m):
        m.density_grid.copy_(occ)
        m.density_bitfield.copy_(bits)
    return dev, batches, keep


def _check_loss(st, loss, target, what):
    img = st.image
    assert img is not None and img.shape == (N_RAYS, 3) and img.dtype == torch.float32 and not img.requires_grad, what
    want = float(((img.double() - target.double()) ** 2).mean())
    rel = abs(float(loss) - want) / want
    print(f'{what}: loss {float(loss):.9g}, mean (image - target)^2 {want:.9g}, relative difference {rel / 2.0 ** -24:.2f} x 2^-24')
    assert rel <= LOSS_RTOL, (what, float(loss), want)


@pytest.mark.parametrize('lookahead', [False, True])
def test_stepper_image_is_the_image_of_the_step(lookahead, scene):
    """after step(), stepper.image is that step's finished image: its squared error against the target is the returned loss (eager first
    steps, three replayed steps, the step that captures a second capacity, the step after the switch back), and it holds the bits
    fused_train_iteration returns for the same batch and parameters (called by hand on the stepper's own static buffers right before the
    step: it deposits gradients but takes no optimizer step, so the replayed step reads the same parameters)"""
    from fused import fused_train_iteration
    from graph import GraphedTrainStep
    dev, batches, keep = scene
    FIRST, BY_HAND, GROW, BACK = 16, 19, 20, 21     # the first replayed step (after 16 eager ones), ...
    model, opt = _make_ngp(dev)
    st = GraphedTrainStep(model, opt, None, N_RAYS, KW, after_update=keep, direct=True, lookahead=lookahead, capacity_quantum=1024,
                          capacity_ladder=())
    assert st.image is None
    for i in range(BACK + 1):
        nxt = dict(next_rays=batches[i + 1]) if lookahead else {}
        by_hand = None
        if i == BY_HAND:
            torch.cuda.synchronize()
            o, d, t = batches[i]
            if lookahead:      # the announced batch is already staged and marched in set la_cur
                p = st.la_cur
                assert st.la_ready[p] is not None and torch.equal(st.la_rays_o[p], o.view(-1, 3)) and torch.equal(st.la_target[p], t)
                args, kwargs = st._iteration_args(st._checked_ok, p)
            else:
                torch._foreach_copy_([st.rays_o, st.rays_d, st.target], [o, d, t])
                args, kwargs = st._iteration_args(st.producers_check)
            by_hand = fused_train_iteration(*args, **kwargs)[1].clone()
        if i == GROW:
            mc = model.mean_count
            model.mean_count = 3 * mc           # the estimate leaves the captured buffer: a second capacity is captured
        if i == BACK:
            model.mean_count = mc               # ... and back: the first capacity's graphs are switched in, nothing is captured
            captures = st.n_captures
        loss = st.step(*batches[i], **nxt)
        if i in (0, 5, FIRST, FIRST + 1, FIRST + 2, BY_HAND, GROW, BACK):
            _check_loss(st, loss, batches[i][2], f'lookahead={lookahead} step {i}')
        if by_hand is not None:
            assert st.graphs is not None and st.capacity == st.captured_capacity
            assert torch.equal(st.image, by_hand)
    assert st.capture_error is None and st.used_direct and st.graphs is not None
    assert (st.la is not None) == lookahead
    assert st.n_switches >= 1 and st.n_captures == captures and len(st._captured) == 2
    st.close()
