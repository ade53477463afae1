"""Volume renderer with the reference NeRFRenderer's surface (nerf/renderer.py:61-574): same constructor, buffers (aabb_train,
aabb_infer, density_grid, density_bitfield, step_counter: checkpoint compatible), `render`, `run_cuda` (occupancy-grid ray
marching, the hot path), `run` (the plain sampler of renderer.py:125-253: uniform + importance samples, cumprod compositing --
BASELINE config 1's algorithm), `update_extra_state`, `mark_untrained_grid`, `reset_extra_state`.

Semantics kept from the reference: training depth is measured from the perturbed start of the ray and then has
`nears` subtracted again (renderer.py:317), inference depth is absolute; the 16-slot step_counter ring and
`mean_count` estimate; density-grid EMA-max update with full sweeps for the first 16 calls and quarter-random +
quarter-occupied resampling afterwards; packbits against min(mean_density, density_thresh).
"""
import math

import numpy as np
import torch
import torch.nn as nn

import raymarching


def _meshgrid(*axes):
    return torch.meshgrid(*axes, indexing='ij')


def sample_pdf(bins, weights, n_samples, det=False):
    """inverse-transform sampling of the piecewise-constant pdf `weights` [B,T-1] over `bins` [B,T] -> [B,n_samples]
    (the NeRF hierarchical sampler, renderer.py:12-46)"""
    pdf = weights + 1e-5
    pdf = pdf / pdf.sum(-1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    if det:
        u = torch.linspace(0.5 / n_samples, 1.0 - 0.5 / n_samples, steps=n_samples, device=weights.device)
        u = u.expand(*cdf.shape[:-1], n_samples)
    else:
        u = torch.rand(*cdf.shape[:-1], n_samples, device=weights.device)
    u = u.contiguous()
    hi = torch.searchsorted(cdf, u, right=True)
    lo = (hi - 1).clamp(min=0)
    hi = hi.clamp(max=cdf.shape[-1] - 1)
    cdf_lo, cdf_hi = torch.gather(cdf, -1, lo), torch.gather(cdf, -1, hi)
    bin_lo, bin_hi = torch.gather(bins, -1, lo), torch.gather(bins, -1, hi)
    width = cdf_hi - cdf_lo
    width = torch.where(width < 1e-5, torch.ones_like(width), width)
    return bin_lo + (u - cdf_lo) / width * (bin_hi - bin_lo)


def _alpha_weights(z_vals, sample_dist, sigma, density_scale):
    """per-sample compositing weights of the plain sampler (renderer.py:181-186, 218-222)"""
    deltas = torch.cat([z_vals[..., 1:] - z_vals[..., :-1], sample_dist * torch.ones_like(z_vals[..., :1])], -1)
    alphas = 1 - torch.exp(-deltas * density_scale * sigma)
    trans = torch.cumprod(torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15], -1), -1)[..., :-1]
    return deltas, alphas * trans


class NeRFRenderer(nn.Module):
    def __init__(self, bound=1, cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01, bg_radius=-1):
        super().__init__()
        self.bound = bound
        self.cascade = 1 + math.ceil(math.log2(bound))
        self.grid_size = 128
        self.density_scale = density_scale
        self.min_near = min_near
        self.density_thresh = density_thresh
        self.bg_radius = bg_radius

        box = torch.FloatTensor([-bound, -bound, -bound, bound, bound, bound])
        self.register_buffer('aabb_train', box)
        self.register_buffer('aabb_infer', box.clone())

        self.cuda_ray = cuda_ray
        if cuda_ray:
            cells = self.grid_size ** 3
            self.register_buffer('density_grid', torch.zeros(self.cascade, cells))
            self.register_buffer('density_bitfield', torch.zeros(self.cascade * cells // 8, dtype=torch.uint8))
            self.register_buffer('step_counter', torch.zeros(16, 2, dtype=torch.int32))
            self._mean_density, self._mean_density_dev = 0.0, None
            self.iter_density = 0
            self.mean_count = 0
            self.local_step = 0

    # -- model hooks (implemented by the network) -----------------------------------------------
    def forward(self, x, d):
        raise NotImplementedError()

    def density(self, x):
        raise NotImplementedError()

    def color(self, x, d, mask=None, **kwargs):
        raise NotImplementedError()

    def reset_extra_state(self):
        if not self.cuda_ray:
            return
        self.density_grid.zero_()
        self.step_counter.zero_()
        self.mean_density = 0
        self.iter_density = 0
        self.mean_count = 0
        self.local_step = 0

    # -- rendering ------------------------------------------------------------------------------
    def run(self, rays_o, rays_d, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """the plain (non-cuda_ray) sampler, renderer.py:125-253: `num_steps` uniform samples between the AABB hits, optionally
        `upsample_steps` importance samples drawn from the coarse weights, density queried for every sample, colour only where the
        weight exceeds 1e-4, cumprod compositing.  rays_o, rays_d [B,N,3] (B == 1) -> image [B,N,3], depth [B,N], weights_sum [N]"""
        lead = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        n_rays, dev = rays_o.shape[0], rays_o.device
        box = self.aabb_train if self.training else self.aabb_infer
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, box, self.min_near)
        nears, fars = nears.unsqueeze(-1), fars.unsqueeze(-1)
        span = fars - nears
        z_vals = nears + span * torch.linspace(0.0, 1.0, num_steps, device=dev).unsqueeze(0).expand(n_rays, num_steps)
        sample_dist = span / num_steps
        if perturb:
            z_vals = z_vals + (torch.rand(z_vals.shape, device=dev) - 0.5) * sample_dist

        def points(z):
            p = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z.unsqueeze(-1)
            return torch.min(torch.max(p, box[:3]), box[3:])

        xyzs = points(z_vals)
        dens = {k: v.view(n_rays, num_steps, -1) for k, v in self.density(xyzs.reshape(-1, 3)).items()}
        if upsample_steps > 0:
            with torch.no_grad():
                deltas, weights = _alpha_weights(z_vals, sample_dist, dens['sigma'].squeeze(-1), self.density_scale)
                mids = z_vals[..., :-1] + 0.5 * deltas[..., :-1]
                new_z = sample_pdf(mids, weights[:, 1:-1], upsample_steps, det=not self.training).detach()
                new_xyzs = points(new_z)
            new_dens = {k: v.view(n_rays, upsample_steps, -1) for k, v in self.density(new_xyzs.reshape(-1, 3)).items()}
            z_vals, order = torch.sort(torch.cat([z_vals, new_z], 1), dim=1)
            xyzs = torch.cat([xyzs, new_xyzs], 1)
            xyzs = torch.gather(xyzs, 1, order.unsqueeze(-1).expand_as(xyzs))
            for k in dens:
                both = torch.cat([dens[k], new_dens[k]], 1)
                dens[k] = torch.gather(both, 1, order.unsqueeze(-1).expand_as(both))
        _, weights = _alpha_weights(z_vals, sample_dist, dens['sigma'].squeeze(-1), self.density_scale)
        dirs = rays_d.view(-1, 1, 3).expand_as(xyzs)
        flat = {k: v.reshape(-1, v.shape[-1]) for k, v in dens.items()}
        rgbs = self.color(xyzs.reshape(-1, 3), dirs.reshape(-1, 3), mask=(weights > 1e-4).reshape(-1), **flat).view(n_rays, -1, 3)
        weights_sum = weights.sum(-1)
        depth = torch.sum(weights * ((z_vals - nears) / span).clamp(0, 1), -1)
        image = torch.sum(weights.unsqueeze(-1) * rgbs, -2)
        image = image + (1 - weights_sum).unsqueeze(-1) * self._background(rays_o, rays_d, bg_color)
        return {'depth': depth.view(*lead), 'image': image.view(*lead, 3), 'weights_sum': weights_sum}

    def _background(self, rays_o, rays_d, bg_color):
        if self.bg_radius > 0:
            sph = raymarching.sph_from_ray(rays_o, rays_d, self.bg_radius)
            # .float(): under autocast the background network returns fp16, and PyTorch-ROCm's same-shape MIXED-dtype elementwise kernel
            # (fp32 gradient x fp16 colour in the backward of the blend below) runs [4096, 3] in ONE workgroup for 45-170 us (4 us for
            # fp32 x fp32; measured in isolation and in the config-5 step, EXPERIMENTS.md round 5).  Same values: the blend promotes to fp32
            # either way, and the gradient is rounded to fp16 once on the way back in both forms.
            return self.background(sph, rays_d).float()
        return 1 if bg_color is None else bg_color

    def _finish(self, image, depth, weights_sum, bg_color, nears, fars, lead):
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        return image.view(*lead, 3), depth.view(*lead)

    def _fused_render_ok(self, rays_o, rays_d, bg_color, force_all_rays, geo=False, aux=None):
        """the fused training render needs the estimate-sized sample buffer (no host read-back), a plain colour background and a
        network the fused sample pipeline accepts (network_ff.NeRFNetwork._fused_ok); it has no geometry outputs (geo) and composites no
        channels of the caller's (aux)"""
        if geo or aux is not None or not getattr(self, 'fused', False) or force_all_rays or self.mean_count <= 0 or self.bg_radius > 0:
            return False
        if not (rays_o.is_cuda and rays_o.dtype == torch.float32 and rays_d.dtype == torch.float32):
            return False
        if torch.is_tensor(bg_color) and (bg_color.numel() != rays_o.shape[0] * 3 or not bg_color.is_cuda):
            return False
        if not (torch.is_tensor(bg_color) or isinstance(bg_color, (int, float))):
            return False
        probe = getattr(self, '_fused_ok', None)
        if probe is None:
            return False
        dummy = torch.empty(128, 3, device=rays_o.device)
        return bool(probe(dummy, dummy)) and torch.is_grad_enabled()

    def run_cuda(self, rays_o, rays_d, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False, max_steps=1024,
                 T_thresh=1e-4, geo=False, aux=None, aux_infer=None, **kwargs):
        # rays_o, rays_d [B, N, 3] (B == 1) -> {'image' [B,N,3], 'depth' [B,N], ('weights_sum' when training)}
        # geo (extension, training only): composite with raymarching.composite_rays_train_geo -- 'depth' becomes differentiable
        # and the results gain 'depth_raw' [N] (the compositor's un-normalised depth) and 'distortion' [N] (EffDistLoss per ray / (far - near))
        # aux (extension, training only): a callable (xyzs, dirs, sigmas, rgbs) -> [M,C] evaluated on the marched samples; the
        # results gain 'aux' [N,C], its raw composite under the rays' weights (raymarching.composite_rays_train_features, no background blend)
        if aux is not None and not self.training:
            raise NotImplementedError("render(aux=...): the 'aux' channels are composited by the training compositor only (model.train()); the "
                                      "inference loop has no feature compositor for this contract -- an eval frame takes aux_infer=fn "
                                      "(called once per loop iteration, no gradient graph)")
        # aux_infer (extension, eval only): a callable (xyzs [R,3], dirs [R,3], sigmas [R] fp32 density-scaled, rgbs [R,3] fp32)
        # -> [R,C] fp32 or fp16, 1 <= C <= 256, called once per loop iteration on the iteration's padded row buffers (rows behind the marched
        # ones hold zero deltas and arbitrary values; their outputs are never read); the results gain 'aux' [*lead, C] fp32, its raw composite
        # under the frame's weights (raymarching.composite_rays_features, no background blend).  A new keyword, not aux=: that one keeps
        # raising in eval, and its callable is called once on all samples with a gradient graph.
        if aux_infer is not None and self.training:
            raise ValueError("render(aux_infer=...): aux_infer is the eval frame's keyword (model.eval()); a training render composites the "
                             "caller's channels with aux=fn")
        lead = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        n_rays = rays_o.shape[0]
        dev = rays_o.device
        box = self.aabb_train if self.training else self.aabb_infer
        results = {}

        if self.training and self.bg_radius <= 0 and self._fused_render_ok(rays_o, rays_d, 1 if bg_color is None else bg_color, force_all_rays, geo, aux):
            bg_color = 1 if bg_color is None else bg_color
            # extension (fused.py): the whole training branch below as one autograd Function, identical arithmetic
            from fused import fused_render_train
            counter = self.step_counter[self.local_step % 16]
            self.local_step += 1
            capacity = self.mean_count + (128 - self.mean_count % 128)  # raymarching.py:200-203
            image, depth, weights_sum = fused_render_train(self, rays_o, rays_d, box, counter, capacity, bg_color, perturb, dt_gamma,
                                                           max_steps, T_thresh)
            results['weights_sum'] = weights_sum
            results['depth'] = depth.view(*lead)
            results['image'] = image.view(*lead, 3)
            return results

        # extension: training rays that require grad.  near / far, the background lookup and the marcher (forward-only ops)
        # see the rays as constants -- the sample parameters do not depend on the pose -- and the marcher's samples become a function of the
        # rays, x = clamp(o + t d) with its t as constants: the same tensors (the forward does not change by a bit), with a backward that
        # carries dL/dxyzs and dL/ddirs to the rays
        ray_grads = self.training and torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad)
        rays_o_in, rays_d_in = rays_o, rays_d
        if ray_grads:
            rays_o, rays_d = rays_o.detach(), rays_d.detach()
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, box, self.min_near)
        bg_color = self._background(rays_o, rays_d, bg_color)
        if self.training:
            counter = self.step_counter[self.local_step % 16]
            counter.zero_()
            self.local_step += 1
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(
                rays_o, rays_d, self.bound, self.density_bitfield, self.cascade, self.grid_size, nears, fars, counter,
                self.mean_count, perturb, 128, force_all_rays, dt_gamma, max_steps)
            if ray_grads:
                ts = raymarching.sample_ts(xyzs, rays_o, rays_d, rays, self.bound)
                xyzs, dirs = raymarching.ray_points(rays_o_in, rays_d_in, ts, rays, self.bound, like=(xyzs, dirs))
            # (a model that sets takes_deltas -- an SDF model, whose density depends on the section length -- is handed the marcher's deltas)
            sigmas, rgbs = self(xyzs, dirs, deltas=deltas) if getattr(self, 'takes_deltas', False) else self(xyzs, dirs)
            sigmas = self.density_scale * sigmas
            if aux is not None:
                if sigmas.dim() == 2:
                    raise NotImplementedError("render(aux=...): 'aux' is not provided for stacked residual models")
                results['aux'] = raymarching.composite_rays_train_features(sigmas, aux(xyzs, dirs, sigmas, rgbs), deltas, rays, T_thresh)
            if geo:
                composite = raymarching.composite_rays_train_geo
            else:
                composite = lambda *a: raymarching.composite_rays_train(*a) + (None,)
            if sigmas.dim() == 2:  # stacked residual models (CCNeRF): composite each
                images, depths, raws, dists = [], [], [], []
                for k in range(sigmas.shape[0]):
                    weights_sum, depth_raw, image, distortion = composite(sigmas[k], rgbs[k], deltas, rays, T_thresh)
                    image, depth = self._finish(image, depth_raw, weights_sum, bg_color, nears, fars, lead)
                    images.append(image)
                    depths.append(depth)
                    raws.append(depth_raw)
                    dists.append(distortion)
                image, depth = torch.stack(images, 0), torch.stack(depths, 0)
                if geo:
                    depth_raw, distortion = torch.stack(raws, 0), torch.stack(dists, 0)
            else:
                weights_sum, depth_raw, image, distortion = composite(sigmas, rgbs, deltas, rays, T_thresh)
                image, depth = self._finish(image, depth_raw, weights_sum, bg_color, nears, fars, lead)
            results['weights_sum'] = weights_sum
            if geo:
                results['depth_raw'] = depth_raw
                # (a ray that misses the box has near = far and no samples: its distortion stays 0 instead of 0 / 0)
                results['distortion'] = distortion / (fars - nears).clamp_min(torch.finfo(torch.float32).tiny)
        else:
            weights_sum = torch.zeros(n_rays, dtype=torch.float32, device=dev)
            depth = torch.zeros(n_rays, dtype=torch.float32, device=dev)
            image = torch.zeros(n_rays, 3, dtype=torch.float32, device=dev)
            rays_t = nears.clone()
            aux_frame = {'out': None} if aux_infer is not None else None   # 'out' [N,C]: zeros at the callable's first call of the frame
            from fused import pinned_half_weights
            with pinned_half_weights(self):  # one fp16 cast of the parameters per frame instead of one per loop iteration
                if getattr(self, 'device_loop', True):
                    self._render_loop_on_device(rays_o, rays_d, nears, fars, rays_t, weights_sum, depth, image, perturb, dt_gamma, max_steps,
                                                T_thresh, aux_infer=aux_infer, aux_frame=aux_frame)
                else:  # the reference's host-driven loop (renderer.py:341-367): one device->host read-back per iteration
                    rays_alive = torch.arange(n_rays, dtype=torch.int32, device=dev)
                    step = 0
                    while step < max_steps:
                        n_alive = rays_alive.shape[0]
                        if n_alive <= 0:
                            break
                        n_step = max(min(n_rays // n_alive, 8), 1)  # more samples per ray and launch as rays die
                        xyzs, dirs, deltas = raymarching.march_rays(
                            n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound, self.density_bitfield, self.cascade,
                            self.grid_size, nears, fars, 128, perturb if step == 0 else False, dt_gamma, max_steps)
                        sigmas, rgbs = self(xyzs, dirs, deltas=deltas) if getattr(self, 'takes_deltas', False) else self(xyzs, dirs)
                        sigmas = self.density_scale * sigmas
                        if aux_infer is not None:   # the fp32 tensors composite_rays' cast would make: both ops read the same values
                            sigmas, rgbs = sigmas.float().contiguous(), rgbs.float().contiguous()
                            feats = self._aux_infer_feats(aux_infer, aux_frame, xyzs, dirs, sigmas, rgbs, n_rays)
                            raymarching.composite_rays_features(n_alive, n_step, rays_alive, sigmas, feats, deltas, weights_sum, aux_frame['out'],
                                                                T_thresh)
                        raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image,
                                                   T_thresh)
                        rays_alive = rays_alive[rays_alive >= 0]
                        step += n_step
            image, depth = self._finish(image, depth, weights_sum, bg_color, nears, fars, lead)
            if aux_infer is not None:
                out = aux_frame['out']   # (None: a frame without a loop iteration, i.e. without rays -- no call, no channel count)
                results['aux'] = torch.zeros(*lead, 0, dtype=torch.float32, device=dev) if out is None else out.view(*lead, out.shape[1])

        results['depth'] = depth
        results['image'] = image
        return results

    @staticmethod
    def _aux_infer_feats(fn, frame, xyzs, dirs, sigmas, rgbs, n_rays):
        """one call of an eval frame's aux_infer callable on an iteration's row buffers -> feats [R,C] (detached, contiguous, fp32 or fp16);
        the first call of the frame fixes C and the dtype and allocates frame['out'] [n_rays,C] as zeros"""
        with torch.no_grad():
            feats = fn(xyzs, dirs, sigmas, rgbs)
        if not torch.is_tensor(feats) or feats.dim() != 2 or feats.shape[0] != xyzs.shape[0] or not 1 <= feats.shape[1] <= 256:
            raise ValueError(f"render(aux_infer=...): the callable must return a [{xyzs.shape[0]}, C] tensor with 1 <= C <= 256 (got "
                             f"{tuple(feats.shape) if torch.is_tensor(feats) else type(feats).__name__})")
        if feats.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"render(aux_infer=...): the callable must return float32 or float16 (got {feats.dtype})")
        if frame['out'] is None:
            frame['out'] = torch.zeros(n_rays, feats.shape[1], dtype=torch.float32, device=xyzs.device)
            frame['dtype'] = feats.dtype
        elif feats.shape[1] != frame['out'].shape[1] or feats.dtype != frame['dtype']:
            raise ValueError(f"render(aux_infer=...): every call of a frame must return the same C and dtype (first call: C = "
                             f"{frame['out'].shape[1]}, {frame['dtype']}; this call: C = {feats.shape[1]}, {feats.dtype})")
        return feats.detach().contiguous()

    def _render_loop_on_device(self, rays_o, rays_d, nears, fars, rays_t, weights_sum, depth, image, perturb, dt_gamma, max_steps, T_thresh,
                               sync_every=8, aux_infer=None, aux_frame=None):
        """the eval loop of run_cuda (renderer.py:341-367) with its state on the device: nerf/render_loop.py; weights_sum, depth
        and image are accumulated in place, same image as the host-driven loop bit for bit"""
        from .render_loop import FrameLoop
        FrameLoop(self, (rays_o, rays_d, nears, fars, rays_t, weights_sum, depth, image), perturb, dt_gamma, max_steps, T_thresh, sync_every,
                  aux_infer, aux_frame).run()

    # -- occupancy grid maintenance -------------------------------------------------------------
    def _cascade_points(self, coords, cas):
        """cell coordinates [n,3] in [0,grid) -> jittered world positions inside the cells of cascade `cas`"""
        unit = 2 * coords.float() / (self.grid_size - 1) - 1
        bound = min(2 ** cas, self.bound)
        half_cell = bound / self.grid_size
        pts = unit * (bound - half_cell)
        pts += (torch.rand_like(pts) * 2 - 1) * half_cell
        return pts

    def _query_sigma(self, pts):
        return self.density(pts)['sigma'].reshape(-1).detach() * self.density_scale

    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsic, S=64):
        """cells no training camera sees get density -1 and are never marked occupied (renderer.py:379-442)"""
        if not self.cuda_ray:
            return
        if isinstance(poses, np.ndarray):
            poses = torch.from_numpy(poses)
        dev = self.density_bitfield.device
        poses = poses.to(dev)
        fx, fy, cx, cy = intrinsic
        n_views = poses.shape[0]
        axis = torch.arange(self.grid_size, dtype=torch.int32, device=dev).split(S)
        count = torch.zeros_like(self.density_grid)
        for xs in axis:
            for ys in axis:
                for zs in axis:
                    xx, yy, zz = _meshgrid(xs, ys, zs)
                    coords = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
                    cell_ids = raymarching.morton3D(coords).long()
                    unit = (2 * coords.float() / (self.grid_size - 1) - 1).unsqueeze(0)
                    for cas in range(self.cascade):
                        bound = min(2 ** cas, self.bound)
                        half_cell = bound / self.grid_size
                        world = unit * (bound - half_cell)
                        for head in range(0, n_views, S):
                            cam = poses[head:head + S]
                            local = (world - cam[:, :3, 3].unsqueeze(1)) @ cam[:, :3, :3]
                            z = local[:, :, 2]
                            seen = (z > 0) & (local[:, :, 0].abs() < cx / fx * z + half_cell * 2) \
                                & (local[:, :, 1].abs() < cy / fy * z + half_cell * 2)
                            count[cas, cell_ids] += seen.sum(0).reshape(-1)
        self.density_grid[count == 0] = -1

    @property
    def mean_density(self):
        """mean of the clamped density grid (renderer.py:527); kept on the device by the refresh and read back only when asked for"""
        if self._mean_density_dev is not None:
            self._mean_density = float(self._mean_density_dev.item())
            self._mean_density_dev = None
        return self._mean_density

    @mean_density.setter
    def mean_density(self, value):
        self._mean_density, self._mean_density_dev = float(value), None

    @torch.no_grad()
    def refresh_sample(self, S=128, full=None):
        """the weight-INDEPENDENT half of the occupancy refresh: which cells are re-evaluated, and where inside them (renderer.py:444-514).
        Full sweep: every cell; else a quarter of the cells at random plus as many drawn from the currently occupied ones -- the
        `torch.nonzero` + random choice of the reference becomes an equivalent draw (uniform over the occupied cells, with replacement)
        through a prefix sum and a binary search, so nothing is read back.  Returns [(cascade, cell ids, jittered world positions)].
        Depends only on the density grid and the random stream: graph.GraphedTrainStep runs it on a side stream under the previous
        training iteration."""
        dev = self.density_bitfield.device
        full = (self.iter_density < 16) if full is None else full
        samples = []
        if full:  # full sweep
            axis = torch.arange(self.grid_size, dtype=torch.int32, device=dev).split(S)
            for xs in axis:
                for ys in axis:
                    for zs in axis:
                        xx, yy, zz = _meshgrid(xs, ys, zs)
                        coords = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
                        cell_ids = raymarching.morton3D(coords).long()
                        for cas in range(self.cascade):
                            samples.append((cas, cell_ids, self._cascade_points(coords, cas)))
        else:  # a quarter of the cells at random plus as many drawn from the currently occupied ones
            # Both draws are i.i.d. uniform WITH replacement, as in the reference -- but generated as ORDER STATISTICS, i.e. already sorted
            # by Morton code: n sorted uniforms are the normalised partial sums of n + 1 exponentials (one cumsum).  The density network then
            # sees spatially coherent points (neighbours in the list are neighbours in space), which is what the encoder's caches want:
            # the refresh is the one place where the hash grid was evaluated on randomly ORDERED points.  Which cells are drawn has the
            # same distribution as before; the scatter of the results does not depend on the order (duplicates: any of them wins, as in
            # the reference).
            n = self.grid_size ** 3 // 4
            cells = self.grid_size ** 3

            def sorted_uniform(count):
                """`count` i.i.d. uniforms on [0, 1), ascending (fp64 partial sums: 2^19 terms)"""
                e = -torch.log(torch.rand(count + 1, device=dev, dtype=torch.float64).clamp_(min=1e-300))
                c = torch.cumsum(e, 0)
                return (c[:count] / c[count]).clamp_(max=1.0 - 2.0 ** -40)
            for cas in range(self.cascade):
                rand_ids = (sorted_uniform(n) * cells).long().clamp_(max=cells - 1)
                rand_coords = raymarching.morton3D_invert(rand_ids)
                # occ_ids = nonzero(grid > 0)[randint(0, count, n)] without knowing `count` on the host
                occupied = torch.cumsum(self.density_grid[cas] > 0, 0, dtype=torch.int32)
                pick = (sorted_uniform(n) * occupied[-1]).to(torch.int32).clamp_(max=occupied[-1] - 1).clamp_(min=0)
                occ_ids = torch.searchsorted(occupied, pick + 1).clamp_(max=occupied.shape[0] - 1)
                occ_coords = raymarching.morton3D_invert(occ_ids)
                cell_ids = torch.cat([rand_ids, occ_ids], 0)
                coords = torch.cat([rand_coords, occ_coords], 0)
                samples.append((cas, cell_ids, self._cascade_points(coords, cas)))
        return samples

    @torch.no_grad()
    def refresh_apply(self, samples, decay=0.95):
        """the weight-dependent half: density at the sampled positions (ONE network evaluation over all cascades), then the EMA-max
        update of the cells that are valid on both sides, the mean of the clamped grid and the bitfield packed against
        min(mean_density, density_thresh) (renderer.py:515-529) as one native call of three launches (raymarching.update_density_grid;
        the reference issues ~15 PyTorch launches over the whole grid here).  No host synchronisation (capturable).  Returns the device
        mean.  `fused_refresh = False` keeps the PyTorch formulation (identical values; tests compare the two)."""
        cells = self.grid_size ** 3
        if getattr(self, 'fused_refresh', True) and self.density_grid.is_cuda and self.density_grid.is_contiguous():
            if len(samples) == 1 and samples[0][0] == 0:
                ids, pts = samples[0][1], samples[0][2]
            else:
                ids = torch.cat([cell_ids + cas * cells for cas, cell_ids, _ in samples], 0)
                pts = torch.cat([p for _, _, p in samples], 0)
            # (refresh_sample hands over Morton-sorted cells: consecutive points are ~ (4 cells per sample)^(1/3) = 1.6 cells apart; in the
            # encoder's unit cube a cell of cascade 0 measures 1 / grid_size -- a hint for the encoder's work-list balancing, nothing else)
            import fused as _fused
            _fused.density_point_spacing = 1.6 / self.grid_size if len(samples) == self.cascade and len(samples[0][1]) < cells else None
            try:
                # ONE network evaluation over all cascades up to REFRESH_CHUNK points, chunked beyond (a full sweep of bound 16 is
                # 5 x 128^3 = 10.5 M points; peak activation memory -- and the pool of a graph the refresh is captured into -- otherwise
                # grows with the cascade count)
                chunk = int(getattr(self, 'refresh_chunk', 1 << 22))
                if pts.shape[0] <= chunk:
                    sigma = self.density(pts)['sigma'].reshape(-1).detach()      # density_scale is applied by the update kernel
                else:
                    sigma = torch.cat([self.density(pts[i:i + chunk])['sigma'].reshape(-1).detach() for i in range(0, pts.shape[0], chunk)], 0)
            finally:
                _fused.density_point_spacing = None
            state = self.__dict__.setdefault('_refresh_state', {})
            return raymarching.update_density_grid(sigma, ids, self.density_scale, decay, self.density_grid, self.density_thresh,
                                                   self.density_bitfield, state).reshape(())
        fresh = -torch.ones_like(self.density_grid)
        for cas, cell_ids, pts in samples:
            fresh[cas, cell_ids] = self._query_sigma(pts)
        # written as a select so that no boolean-index gather/scatter (and its host synchronisation) is needed: identical values
        both = (self.density_grid >= 0) & (fresh >= 0)
        self.density_grid.copy_(torch.where(both, torch.maximum(self.density_grid * decay, fresh), self.density_grid))
        mean = torch.mean(self.density_grid.clamp(min=0))
        raymarching.packbits_capped(self.density_grid, self.density_thresh, mean, self.density_bitfield)
        return mean

    @torch.no_grad()
    def refresh_occupancy(self, decay=0.95, S=128, full=None):
        """the device part of update_extra_state (renderer.py:444-529): refresh_sample + refresh_apply"""
        return self.refresh_apply(self.refresh_sample(S, full), decay)

    def finish_update(self, mean, mean_count=None):
        """the host part of update_extra_state: bookkeeping and the sample-count estimate (one read-back, renderer.py:531-538).
        mean_count: the estimate when the caller has read the counter ring already (graph.GraphedTrainStep reads it off the main stream)"""
        self._mean_density_dev = mean.detach().reshape(())
        self.iter_density += 1
        used = min(16, self.local_step)
        if used > 0:
            self.mean_count = int(self.step_counter[:used, 0].sum().item() / used) if mean_count is None else int(mean_count)
        self.local_step = 0

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=128):
        """refresh the density grid / bitfield and the sample-count estimate (renderer.py:444-538)"""
        if not self.cuda_ray:
            return
        self.finish_update(self.refresh_occupancy(decay, S))

    # -- mesh extraction (extension) ---------------------------------------------
    # the scalar field extract_mesh contours: density(x)['sigma'] * density_scale, inside ABOVE the level (default 10, the reference's
    # save_mesh threshold), unevaluated lattice points hold 0.  A model with another field overrides the three attributes and _mesh_values
    # (network_sdf.py).
    mesh_level, mesh_inside_below, mesh_fill = 10.0, False, 0.0

    def _mesh_values(self, pts):
        return self._query_sigma(pts).float()

    @torch.no_grad()
    def mesh_volume(self, dims, lo, hi, cull=True, fill=None, slab_points=2 ** 24):
        """the fill of extract_mesh alone: the model's field on the lattice dims = (nx, ny, nz) over [lo, hi] -> (volume [nz,ny,nx] fp32, the
        number of lattice points evaluated).  z-slab by z-slab of at most `slab_points` points: raymarching.lattice_points names the points
        (cull: those within one occupancy cell of a set bit of density_bitfield; else all), the field is evaluated on them in eval mode under
        fp16 autocast (the numerics a frame is rendered with) and scattered by index into a volume prefilled with `fill`."""
        if cull and not self.cuda_ray:
            raise RuntimeError("extract_mesh(cull=True) reads the occupancy bitfield of a cuda_ray model; pass cull=False")
        nx, ny, nz = dims
        dev = self.aabb_train.device
        volume = torch.full((nz, ny, nx), float(self.mesh_fill if fill is None else fill), dtype=torch.float32, device=dev)
        flat = volume.view(-1)
        slab = max(1, int(slab_points) // (nx * ny))
        bits = self.density_bitfield if cull else None
        evaluated = 0
        was_training = self.training
        self.eval()
        try:
            with torch.autocast('cuda', dtype=torch.float16, enabled=dev.type == 'cuda'):
                for z0 in range(0, nz, slab):
                    pts, index = raymarching.lattice_points(lo, hi, dims, z0, min(z0 + slab, nz), bits, self.bound, self.cascade, self.grid_size,
                                                            1, device=dev)
                    if pts.shape[0]:
                        flat[index.long()] = self._mesh_values(pts).reshape(-1)
                        evaluated += pts.shape[0]
        finally:
            self.train(was_training)
        return volume, evaluated

    def extract_mesh(self, resolution=256, level=None, lo=None, hi=None, cull=True, fill=None, slab_points=2 ** 24, return_volume=False):
        """the level set of the model's field as an indexed triangle mesh -> (vertices [V,3] fp32 world positions, faces [F,3] int32), plus
        the volume [nz,ny,nx] with return_volume.  The field is evaluated on the lattice of `resolution` (an int or (nx, ny, nz)) points
        spanning [lo, hi] (default +-bound) by mesh_volume -- cull=True: only near occupied space, which needs cuda_ray -- and contoured by
        raymarching.surface_nets at `level` (default: the model's mesh_level).  No gradient."""
        dims = [int(resolution)] * 3 if not hasattr(resolution, '__len__') else [int(n) for n in resolution]
        if len(dims) != 3 or min(dims) < 2:
            raise ValueError(f"extract_mesh: resolution must be an int or (nx, ny, nz), each at least 2 (got {resolution})")
        lo = -self.bound if lo is None else lo
        hi = self.bound if hi is None else hi
        volume, _ = self.mesh_volume(dims, lo, hi, cull, fill, slab_points)
        origin, spacing = raymarching.lattice_frame(lo, hi, dims)
        vertices, faces = raymarching.surface_nets(volume, self.mesh_level if level is None else level, self.mesh_inside_below, origin, spacing)
        return (vertices, faces, volume) if return_volume else (vertices, faces)

    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """renderer.py:540-574: run_cuda with cuda_ray (never staged), else `run`, in ray batches of `max_ray_batch` when staged"""
        if kwargs.get('aux') is not None and (staged or not self.cuda_ray):
            raise NotImplementedError("render(aux=...): the 'aux' channels need the cuda_ray training render; the staged / non-cuda_ray path "
                                      "does not composite them")
        if kwargs.get('aux_infer') is not None and not self.cuda_ray:
            raise NotImplementedError("render(aux_infer=...): the 'aux' channels of an eval frame are composited by the cuda_ray inference loop; "
                                      "the non-cuda_ray path does not composite them")
        if self.cuda_ray:
            return self.run_cuda(rays_o, rays_d, **kwargs)
        if not staged:
            return self.run(rays_o, rays_d, **kwargs)
        B, N = rays_o.shape[:2]
        depth = torch.empty(B, N, device=rays_o.device)
        image = torch.empty(B, N, 3, device=rays_o.device)
        for b in range(B):
            for head in range(0, N, max_ray_batch):
                tail = min(head + max_ray_batch, N)
                part = self.run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], **kwargs)
                depth[b:b + 1, head:tail] = part['depth']
                image[b:b + 1, head:tail] = part['image']
        return {'depth': depth, 'image': image}
