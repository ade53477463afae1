"""GPU checks of nerf.network_sdf.NeuSNetwork: the first in-tree consumer of the second-order stack end to end -- hash grid ->
FFMLP -> grad sdf with create_graph -> raymarching.sdf_sigmas -> the training compositor (geo=True, aux= the normals) -> loss -> backward,
plus an eikonal term; an eval frame with aux_infer= through the per-stage device loop; and 100 steps of Adam with the fused op against the
same model with the plain-torch chain of the definition patched in.

Scene: an analytic sphere of radius 0.35 with a shaded colour on a white background, 256 rays; the model's sphere prior has radius 0.6, so
the surface has to move.  Tiny model: 2^12 table entries per level, bound 1."""
import numpy as np
import pytest
import torch

import sdf_sigmas_cases as C

pytestmark = pytest.mark.gpu

RADIUS, PRIOR_RADIUS, N_RAYS, MAX_STEPS = 0.35, 0.6, 256, 256
LIGHT = np.array([0.3, 0.5, -0.81])
BASE = np.array([0.9, 0.5, 0.2])


def _scene(seed=3):
    """256 rays from a sphere of radius 1.8 towards a disk of radius 0.6 around the origin -> rays_o, rays_d, gt [N,3] (float32 cuda)"""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(N_RAYS, 3))
    o *= 1.8 / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.normal(size=(N_RAYS, 3))
    target -= (target * o).sum(1, keepdims=True) * o / 1.8 ** 2          # in the plane through the origin across the view direction
    target *= (0.6 * np.sqrt(rng.uniform(0, 1, (N_RAYS, 1)))) / np.linalg.norm(target, axis=1, keepdims=True)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = -(o * d).sum(1)
    disc = b * b - ((o * o).sum(1) - RADIUS ** 2)
    hit = disc > 0
    t = b - np.sqrt(np.where(hit, disc, 0.0))
    n = (o + t[:, None] * d) / RADIUS
    shade = 0.2 + 0.8 * np.clip((n * (-LIGHT / np.linalg.norm(LIGHT))).sum(1), 0.0, 1.0)
    gt = np.where(hit[:, None], shade[:, None] * BASE[None, :], 1.0)
    assert 40 < hit.sum() < N_RAYS - 40
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    return f32(o), f32(d), f32(gt)


def _model(seed=0):
    from nerf.network_sdf import NeuSNetwork
    torch.manual_seed(seed)
    model = NeuSNetwork(bound=1, cuda_ray=True, log2_hashmap_size=12, prior_radius=PRIOR_RADIUS, deterministic=True).cuda()
    with torch.autocast('cuda', dtype=torch.float16):
        model.update_extra_state()          # the occupancy grid from density(): inv_s (1 - sigmoid(inv_s f))
    bits = model.density_bitfield
    assert (bits != 0).any() and (bits == 0).any()   # the prior sphere is occupied, the corners of the box are not
    return model


def _step(model, scene, eik_seed):
    """one training step's losses -> (total loss, photometric loss, render results)"""
    rays_o, rays_d, gt = scene
    gen = torch.Generator(device='cuda').manual_seed(eik_seed)
    with torch.autocast('cuda', dtype=torch.float16):
        out = model.render(rays_o[None], rays_d[None], staged=False, bg_color=1, perturb=False, force_all_rays=True, dt_gamma=0,
                           max_steps=MAX_STEPS, geo=True, aux=lambda x, d, s, c: model.last_normals)
        photometric = ((out['image'][0] - gt) ** 2).mean()
        pts = torch.rand(1024, 3, device='cuda', generator=gen) * 2 - 1
        _, normals = model.sdf_and_normal(pts)
        eikonal = ((normals.float().norm(dim=-1) - 1.0) ** 2).mean()
        loss = photometric + 0.1 * eikonal + 0.01 * out['distortion'].mean() + 1e-3 * (out['aux'] ** 2).mean()
    return loss, photometric, out


def _one_step_grads(seed):
    model, scene = _model(seed), _scene()
    model.train()
    loss, _, out = _step(model, scene, 11)
    loss.backward()
    torch.cuda.synchronize()
    return model, loss.detach(), out


def test_training_step_reaches_every_parameter_and_repeats_bit_for_bit():
    (m1, l1, out), (m2, l2, _) = _one_step_grads(0), _one_step_grads(0)
    assert torch.isfinite(l1) and out['aux'].shape == (N_RAYS, 3) and out['distortion'].shape == (N_RAYS,)
    assert int(m1.step_counter[0, 0]) > N_RAYS            # the rays found samples
    for name in ('encoder.embeddings', 'sdf_net.weights', 'color_net.weights', 'log_inv_s'):
        g1, g2 = dict(m1.named_parameters())[name].grad, dict(m2.named_parameters())[name].grad
        assert g1 is not None and torch.isfinite(g1).all() and g1.abs().sum() > 0, name
        assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), name
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))


def test_eval_frame_with_aux_infer():
    model = _model(0).eval()
    side = 32
    u = torch.linspace(-0.95, 0.95, side, device='cuda')
    uu, vv = torch.meshgrid(u, u, indexing='ij')
    rays_o = torch.stack([uu, vv, torch.full_like(uu, -1.5)], -1).reshape(1, -1, 3)
    rays_d = torch.tensor([0.0, 0.0, 1.0], device='cuda').expand_as(rays_o).contiguous()
    calls = []

    def normal_map(x, d, s, c):
        calls.append(x.shape[0])
        return model.last_normals

    with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
        out = model.render(rays_o, rays_d, staged=False, bg_color=1, perturb=False, dt_gamma=0, max_steps=MAX_STEPS, aux_infer=normal_map)
    assert out['image'].shape == (1, side * side, 3) and out['aux'].shape == (1, side * side, 3) and len(calls) >= 2
    assert torch.isfinite(out['image']).all() and torch.isfinite(out['aux']).all()
    impact = (uu ** 2 + vv ** 2).sqrt().reshape(-1)
    frame_weights = _frame_weights(model, rays_o, rays_d)   # (an eval frame does not return weights_sum)
    inner, outer = impact < 0.5 * PRIOR_RADIUS, impact > PRIOR_RADIUS + 0.1
    assert int(inner.sum()) > 50 and int(outer.sum()) > 50
    assert (frame_weights[inner] > 0.5).all() and (frame_weights[outer] < 0.5).all()
    # the composited normal of a ray through the sphere looks back at the camera
    assert (out['aux'][0][inner][:, 2] < 0).all()


def _frame_weights(model, rays_o, rays_d):
    """weights_sum of an eval frame: the channel of ones of aux_infer (raymarching.composite_rays_features: a channel of ones gives weights_sum)"""
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
        out = model.render(rays_o, rays_d, staged=False, bg_color=1, perturb=False, dt_gamma=0, max_steps=MAX_STEPS,
                           aux_infer=lambda x, d, s, c: torch.ones(x.shape[0], 1, device=x.device))
    return out['aux'][0, :, 0]


def _train(steps, patch=None):
    """`steps` of Adam on a freshly seeded model -> the photometric loss of every step (one read-back at the end)"""
    import raymarching
    model, scene = _model(0), _scene()
    model.train()
    opt = torch.optim.Adam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    original = raymarching.sdf_sigmas
    if patch is not None:
        raymarching.sdf_sigmas = patch
    try:
        history = []
        for i in range(steps):
            opt.zero_grad(set_to_none=True)
            loss, photometric, _ = _step(model, scene, 100 + i)
            loss.backward()
            opt.step()
            history.append(photometric.detach())
    finally:
        raymarching.sdf_sigmas = original
    return torch.stack(history).cpu().numpy()


def test_fused_op_trains_like_the_torch_chain():
    """The op against its reference inside the model: the same seed, 100 steps of Adam each, the fused op in one run and the plain-torch chain
    of the definition (sdf_sigmas_cases.definition) in the other.  The two differ by rounding only, and the runs are chaotic in the last bits,
    not in the trend: both fall from step 0 and the fused run ends within a factor 2 of the chain's final photometric loss.
    Measured on MI355X: see DESIGN.md 3.16."""
    fused = _train(100)
    chain = _train(100, patch=C.definition)
    ratio = float(fused[-1] / chain[-1])
    print(f'PARITY NeuSNetwork 100 Adam steps: photometric loss fused {fused[0]:.4g} -> {fused[-1]:.4g}, torch chain {chain[0]:.4g} -> {chain[-1]:.4g}, '
          f'ratio {ratio:.3f}')
    assert np.isfinite(fused).all() and np.isfinite(chain).all()
    assert fused[-1] < fused[0] and chain[-1] < chain[0]
    assert abs(float(fused[0]) - float(chain[0])) <= 1e-3 * float(chain[0])   # step 0: the same model, rounding apart
    assert ratio <= 2.0, ratio
