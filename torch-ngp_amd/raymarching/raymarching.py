"""Ray marching / compositing operators with the reference's module-level surface
(raymarching/raymarching.py:19-373): near_far_from_aabb, sph_from_ray, morton3D, morton3D_invert,
packbits, march_rays_train, composite_rays_train, march_rays, composite_rays -- positional
signatures unchanged, so nerf/renderer.py calls them as before (renderer.py:268,286,315,353,361,530).

All floating inputs are cast to fp32 on entry (custom_fwd(cast_inputs=float32)), as in the reference.
Sample slots of march_rays_train are allocated deterministically in ray order by the kernels; the
only host synchronisation left in this file is the one the reference has too (reading the sample
count back when the sample buffer was sized for the worst case, raymarching.py:223-231).
"""
import torch
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

try:  # the compiled binding first, as the reference does (raymarching/raymarching.py:9-12); the ctypes binding of the same C ABI otherwise
    import os as _os
    if _os.environ.get('NGP_HIP_LIBRARY'):  # a variant library is selected: the compiled module links the in-tree one, the ctypes binding follows the variable
        raise ImportError('NGP_HIP_LIBRARY is set')
    import _raymarching as _backend
except ImportError:
    from .backend import _backend
from . import backend as _geo  # the geometry compositor's entries are ctypes-only: the compiled module's table is the reference's

__all__ = ['near_far_from_aabb', 'sph_from_ray', 'morton3D', 'morton3D_invert', 'packbits', 'packbits_capped', 'march_rays_train',
           'composite_rays_train', 'composite_rays_train_geo', 'composite_rays_train_features', 'sample_ts', 'ray_points', 'march_rays', 'composite_rays', 'composite_rays_features', 'compact_rays', 'update_density_grid', 'density_grid_state',
           'sdf_sigmas', 'surface_nets', 'lattice_points', 'lattice_frame']

_f32_fwd = custom_fwd(device_type='cuda', cast_inputs=torch.float32)


def _rays(t):
    t = t if t.is_cuda else t.cuda()
    return t.contiguous().view(-1, 3)


def _round_up_strict(count, align):
    """the reference's padding rule: always adds, a full `align` when already aligned (raymarching.py:200-203)"""
    return count + (align - count % align) if align > 0 else count


# ----------------------------------------------------------------------------------------------
# utilities
# ----------------------------------------------------------------------------------------------
class _near_far_from_aabb(Function):
    @staticmethod
    @_f32_fwd
    def forward(ctx, rays_o, rays_d, aabb, min_near=0.2):
        """rays_o/d [N,3], aabb [6] (xmin,ymin,zmin,xmax,ymax,zmax) -> nears, fars [N]; a miss yields FLT_MAX for both
        (DBL_MAX for float64 tensors)"""
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        n_rays = rays_o.shape[0]
        nears = torch.empty(n_rays, dtype=rays_o.dtype, device=rays_o.device)
        fars = torch.empty_like(nears)
        _backend.near_far_from_aabb(rays_o, rays_d, aabb.contiguous(), n_rays, min_near, nears, fars)
        return nears, fars


near_far_from_aabb = _near_far_from_aabb.apply


class _sph_from_ray(Function):
    @staticmethod
    @_f32_fwd
    def forward(ctx, rays_o, rays_d, radius):
        """far intersection with the sphere of `radius` -> (theta, phi) in [-1, 1]^2, [N, 2]"""
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        n_rays = rays_o.shape[0]
        coords = torch.empty(n_rays, 2, dtype=rays_o.dtype, device=rays_o.device)
        _backend.sph_from_ray(rays_o, rays_d, radius, n_rays, coords)
        return coords


sph_from_ray = _sph_from_ray.apply


class _morton3D(Function):
    @staticmethod
    def forward(ctx, coords):
        """[N,3] int coords in [0,1024) -> [N] int32 interleaved codes"""
        coords = coords if coords.is_cuda else coords.cuda()
        n = coords.shape[0]
        indices = torch.empty(n, dtype=torch.int32, device=coords.device)
        _backend.morton3D(coords.int().contiguous(), n, indices)
        return indices


morton3D = _morton3D.apply


class _morton3D_invert(Function):
    @staticmethod
    def forward(ctx, indices):
        """[N] codes -> [N,3] int32 coords"""
        indices = indices if indices.is_cuda else indices.cuda()
        n = indices.shape[0]
        coords = torch.empty(n, 3, dtype=torch.int32, device=indices.device)
        _backend.morton3D_invert(indices.int().contiguous(), n, coords)
        return coords


morton3D_invert = _morton3D_invert.apply


class _packbits(Function):
    @staticmethod
    @_f32_fwd
    def forward(ctx, grid, thresh, bitfield=None):
        """density grid [C, H^3] -> bitfield [C*H^3/8] uint8, bit i of byte n = grid[8n+i] > thresh (written in place when given)"""
        grid = (grid if grid.is_cuda else grid.cuda()).contiguous()
        n_bytes = grid.shape[0] * grid.shape[1] // 8
        if bitfield is None:
            bitfield = torch.empty(n_bytes, dtype=torch.uint8, device=grid.device)
        _backend.packbits(grid, n_bytes, thresh, bitfield)
        return bitfield


packbits = _packbits.apply


def packbits_capped(grid, thresh, thresh_cap, bitfield):
    """extension (not in the reference): packbits against min(thresh, thresh_cap) where thresh_cap is a 0-dim / 1-element float32
    DEVICE tensor -- the occupancy refresh uses the mean density as the cap without reading it back (no host synchronisation, so the
    refresh can be captured in a HIP graph).  Writes `bitfield` in place and returns it."""
    grid = grid.contiguous()
    n_bytes = grid.shape[0] * grid.shape[1] // 8
    _backend.packbits_capped(grid, n_bytes, float(thresh), thresh_cap.reshape(1).float().contiguous(), bitfield)
    return bitfield


def density_grid_state(density_grid, state):
    """(re)create the buffers `update_density_grid` keeps between calls -- a scratch grid holding -1, the mean's block partials, the device
    mean -- for this grid's size and device.  Call it once OUTSIDE stream capture before the update is captured into a HIP graph (a
    creation inside the capture would be replayed, and re-initialise the buffers, with every replay)."""
    n_cells, dev = density_grid.numel(), density_grid.device
    if state.get('n_cells') != n_cells or state.get('device') != dev:
        if density_grid.is_cuda and torch.cuda.is_current_stream_capturing():
            #  created under a capture the fills below would be REPLAYED, i.e. the scratch grid, the partials and the mean would
            # be re-initialised by every replay -- silently wrong from the second replay on
            raise RuntimeError('density_grid_state: the refresh scratch must be created outside stream capture (call '
                               'raymarching.density_grid_state(model.density_grid, state) -- or run one refresh eagerly -- before capturing)')
        state.update(n_cells=n_cells, device=dev, scratch=torch.full((n_cells,), -1.0, dtype=torch.float32, device=dev),
                     workspace=torch.zeros(int(_backend.density_grid_update_workspace_bytes(n_cells)), dtype=torch.uint8, device=dev),
                     mean=torch.zeros(1, dtype=torch.float32, device=dev))
    return state


def update_density_grid(sigmas, cells, density_scale, decay, density_grid, density_thresh, bitfield, state):
    """extension (not in the reference): the apply half of NeRFRenderer.update_extra_state (nerf/renderer.py:515-529) as one native call --
    `tmp_grid[cas, indices] = density_scale * sigmas`, `grid = max(grid * decay, tmp_grid)` where both are >= 0, the mean of the clamped
    grid and packbits against min(density_thresh, mean) -- without host synchronisation.  cells: int64 GLOBAL cell index (cascade * H^3 +
    morton index) per sigma; `state`: dict owned by the caller that keeps the scratch buffers between calls.
    Writes density_grid / bitfield in place, returns the device mean (1-element fp32 tensor)."""
    n_cells = density_grid.numel()
    density_grid_state(density_grid, state)
    sigmas = sigmas.reshape(-1).float().contiguous()
    cells = cells.reshape(-1).contiguous()
    _backend.density_grid_update(sigmas, cells, sigmas.numel(), float(density_scale), float(decay), density_grid, n_cells, state['scratch'],
                                 float(density_thresh), state['mean'], bitfield, state['workspace'])
    return state['mean']


# ----------------------------------------------------------------------------------------------
# training
# ----------------------------------------------------------------------------------------------
class _march_rays_train(Function):
    @staticmethod
    @_f32_fwd
    def forward(ctx, rays_o, rays_d, bound, density_bitfield, C, H, nears, fars, step_counter=None, mean_count=-1, perturb=False,
                align=-1, force_all_rays=False, dt_gamma=0, max_steps=1024):
        """-> xyzs [M,3], dirs [M,3], deltas [M,2], rays [N,3] = (ray id, first sample, sample count).
        M = mean_count rounded up when a running estimate exists (rays that do not fit are dropped, as in the
        reference), else N*max_steps trimmed to the counted total."""
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        bitfield = (density_bitfield if density_bitfield.is_cuda else density_bitfield.cuda()).contiguous()
        dev, n_rays = rays_o.device, rays_o.shape[0]

        estimated = (not force_all_rays) and mean_count > 0
        capacity = _round_up_strict(mean_count, align) if estimated else n_rays * max_steps

        xyzs = torch.zeros(capacity, 3, dtype=torch.float32, device=dev)
        dirs = torch.zeros(capacity, 3, dtype=torch.float32, device=dev)
        deltas = torch.zeros(capacity, 2, dtype=torch.float32, device=dev)
        rays = torch.empty(n_rays, 3, dtype=torch.int32, device=dev)
        if step_counter is None:
            step_counter = torch.zeros(2, dtype=torch.int32, device=dev)
        noises = torch.rand(n_rays, dtype=torch.float32, device=dev) if perturb else torch.zeros(n_rays, dtype=torch.float32, device=dev)

        _backend.march_rays_train(rays_o, rays_d, bitfield, bound, dt_gamma, max_steps, n_rays, C, H, capacity, nears, fars, xyzs,
                                  dirs, deltas, rays, step_counter, noises)

        if not estimated:
            used = _round_up_strict(int(step_counter[0].item()), align)  # the reference's D2H read (raymarching.py:224)
            xyzs, dirs, deltas = xyzs[:used], dirs[:used], deltas[:used]
        return xyzs, dirs, deltas, rays


march_rays_train = _march_rays_train.apply


class _composite_rays_train(Function):
    @staticmethod
    @_f32_fwd
    def forward(ctx, sigmas, rgbs, deltas, rays, T_thresh=1e-4):
        """sigmas [M], rgbs [M,3], deltas [M,2], rays [N,3] -> weights_sum [N], depth [N], image [N,3]"""
        sigmas, rgbs, deltas = sigmas.contiguous(), rgbs.contiguous(), deltas.contiguous()
        n_samples, n_rays = sigmas.shape[0], rays.shape[0]
        weights_sum = torch.empty(n_rays, dtype=sigmas.dtype, device=sigmas.device)
        depth = torch.empty_like(weights_sum)
        image = torch.empty(n_rays, 3, dtype=sigmas.dtype, device=sigmas.device)
        _backend.composite_rays_train_forward(sigmas, rgbs, deltas, rays, n_samples, n_rays, T_thresh, weights_sum, depth, image)
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, image)
        ctx.sizes = (n_samples, n_rays, T_thresh)
        return weights_sum, depth, image

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, grad_weights_sum, grad_depth, grad_image):
        # grad_depth is not propagated (raymarching.py:275)
        sigmas, rgbs, deltas, rays, weights_sum, image = ctx.saved_tensors
        n_samples, n_rays, T_thresh = ctx.sizes
        grad_sigmas = torch.zeros_like(sigmas)
        grad_rgbs = torch.zeros_like(rgbs)
        _backend.composite_rays_train_backward(grad_weights_sum.contiguous(), grad_image.contiguous(), sigmas, rgbs, deltas, rays,
                                               weights_sum, image, n_samples, n_rays, T_thresh, grad_sigmas, grad_rgbs)
        return grad_sigmas, grad_rgbs, None, None, None


composite_rays_train = _composite_rays_train.apply


class _composite_rays_train_geo(Function):
    """Extension (not in the reference): composite_rays_train for geometry losses.  The same weights_sum, depth and image
    (the same bits) plus the per-ray distortion of loss.py::EffDistLoss on the compositor's own weights, and a backward that propagates
    the gradients of all four outputs -- depth included -- to sigmas and rgbs.  First order only."""

    @staticmethod
    @_f32_fwd
    def forward(ctx, sigmas, rgbs, deltas, rays, T_thresh=1e-4):
        """sigmas [M], rgbs [M,3], deltas [M,2], rays [N,3] -> weights_sum [N], depth [N], image [N,3], distortion [N]"""
        sigmas, rgbs, deltas = sigmas.contiguous(), rgbs.contiguous(), deltas.contiguous()
        n_samples, n_rays = sigmas.shape[0], rays.shape[0]
        weights_sum = torch.empty(n_rays, dtype=sigmas.dtype, device=sigmas.device)
        depth = torch.empty_like(weights_sum)
        distortion = torch.empty_like(weights_sum)
        image = torch.empty(n_rays, 3, dtype=sigmas.dtype, device=sigmas.device)
        _geo.composite_rays_train_geo_forward(sigmas, rgbs, deltas, rays, n_samples, n_rays, T_thresh, weights_sum, depth, image, distortion)
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, depth, image, distortion)
        ctx.sizes = (n_samples, n_rays, T_thresh)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None and goes to the kernel as a NULL pointer
        return weights_sum, depth, image, distortion

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, grad_weights_sum, grad_depth, grad_image, grad_distortion):
        if torch.is_grad_enabled() and any(g is not None and g.requires_grad for g in (grad_weights_sum, grad_depth, grad_image, grad_distortion)):
            raise RuntimeError("composite_rays_train_geo: second-order gradients are not provided (the compositor's backward is not "
                               "differentiable; raymarching stays first-order)")
        sigmas, rgbs, deltas, rays, weights_sum, depth, image, distortion = ctx.saved_tensors
        n_samples, n_rays, T_thresh = ctx.sizes
        grad_sigmas = torch.zeros_like(sigmas)
        grad_rgbs = torch.zeros_like(rgbs)
        dense = lambda g: None if g is None else g.contiguous()
        _geo.composite_rays_train_geo_backward(dense(grad_weights_sum), dense(grad_depth), dense(grad_image), dense(grad_distortion), sigmas, rgbs,
                                               deltas, rays, weights_sum, depth, image, distortion, n_samples, n_rays, T_thresh, grad_sigmas,
                                               grad_rgbs)
        return grad_sigmas, grad_rgbs, None, None, None


composite_rays_train_geo = _composite_rays_train_geo.apply


class _composite_rays_train_features(Function):
    """Extension (not in the reference): composite arbitrary per-sample channels with the volume-rendering weights of
    composite_rays_train,  out[n, c] = sum_i w_i feats[i, c]  over the samples ray n composites -- a normal map, semantic logits, a distilled
    feature field, any per-sample regulariser -- in one launch each way for 1 <= C <= 256 channels, without materialising the weights.
    A channel of ones gives weights_sum; dividing by it gives the expectation of the channels under the ray's weights.  No background is
    blended in.  float64 goes in and out as float64.  Otherwise sigmas and deltas are taken as float32 and out is float32, while float16
    features stay float16 (also under autocast; they are converted at the load and accumulated in float32) and get a float16 gradient.
    First order only; features that come out of a create_graph=True gradient are fine (grad_feats flows back into that graph)."""

    @staticmethod
    def forward(ctx, sigmas, feats, deltas, rays, T_thresh=1e-4):
        """sigmas [M], feats [M,C], deltas [M,2], rays [N,3] -> out [N,C]"""
        if sigmas.dtype == torch.float64 or feats.dtype == torch.float64 or deltas.dtype == torch.float64:
            sigmas, feats, deltas = sigmas.double(), feats.double(), deltas.double()
        else:  # no custom_fwd cast: it would up-cast float16 features
            sigmas, deltas = sigmas.float(), deltas.float()
            feats = feats if feats.dtype == torch.float16 else feats.float()
        if feats.dim() != 2 or feats.shape[0] != sigmas.shape[0]:
            raise RuntimeError(f"composite_rays_train_features: feats must be [M,C] with M = {sigmas.shape[0]} (got {tuple(feats.shape)})")
        sigmas, feats, deltas = sigmas.contiguous(), feats.contiguous(), deltas.contiguous()
        n_samples, n_rays, n_ch = sigmas.shape[0], rays.shape[0], feats.shape[1]
        # every ray's row is written by the kernel; without samples nothing is launched
        out = (torch.zeros if n_samples == 0 else torch.empty)(n_rays, n_ch, dtype=sigmas.dtype, device=sigmas.device)
        _geo.composite_rays_train_features_forward(sigmas, feats, deltas, rays, n_samples, n_rays, n_ch, T_thresh, out)
        ctx.save_for_backward(sigmas, feats, deltas, rays, out)
        ctx.sizes = (n_samples, n_rays, n_ch, T_thresh)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if torch.is_grad_enabled() and grad_out.requires_grad:
            raise RuntimeError("composite_rays_train_features: second-order gradients are not provided (the compositor's backward is not "
                               "differentiable; raymarching stays first-order)")
        sigmas, feats, deltas, rays, out = ctx.saved_tensors
        n_samples, n_rays, n_ch, T_thresh = ctx.sizes
        grad_sigmas = torch.zeros_like(sigmas)
        grad_feats = torch.zeros_like(feats)
        _geo.composite_rays_train_features_backward(grad_out.to(out.dtype).contiguous(), sigmas, feats, deltas, rays, out, n_samples, n_rays, n_ch,
                                                    T_thresh, grad_sigmas, grad_feats)
        return grad_sigmas, grad_feats, None, None, None


composite_rays_train_features = _composite_rays_train_features.apply


class _sdf_sigmas(Function):
    """Extension (not in the reference): render a signed-distance field with the compositors as they are.  NeuS's section
    opacity alpha = clip((prev - next + 1e-5) / (prev + 1e-5), 0, 1), prev / next = sigmoid(inv_s (sdf -+ h)), h = 0.5 ic deltas[:,0] with
    NeuS's annealed cosine ic <= 0 of c = dirs . normals, expressed as the density every compositor turns back into that alpha:
    sigma = min(-log(1 - alpha), 15) / deltas[:,0] in the cancellation-free form log(prev + 1e-5) + softplus(-inv_s (sdf + h)); 0 where
    deltas[:,0] == 0.  One launch each way.  Gradients go to sdf, normals, inv_s and -- when it requires grad -- dirs; capped and padding rows
    get zeros; grad_inv_s is summed in a fixed order (the same bits on every run).  float64 goes in and out as float64, everything else is
    taken as float32.  First order only; normals that come out of a create_graph=True gradient are fine (grad_normals flows back into
    that graph)."""

    @staticmethod
    def forward(ctx, sdf, normals, dirs, deltas, inv_s, cos_anneal=1.0):
        """sdf [M], normals [M,3], dirs [M,3], deltas [M,2], inv_s [1] device tensor, cos_anneal host float in [0, 1] -> sigmas [M]"""
        tensors = (sdf, normals, dirs, deltas, inv_s)
        ctx.like = tuple((t.shape, t.dtype) for t in tensors)
        dtype = _ray_dtype(*tensors)
        n_samples = deltas.shape[0]
        if sdf.numel() != n_samples or tuple(normals.shape) != (n_samples, 3) or tuple(dirs.shape) != (n_samples, 3) or deltas.dim() != 2 or \
                deltas.shape[1] != 2 or inv_s.numel() != 1:
            raise RuntimeError(f"sdf_sigmas: expected sdf [M], normals [M,3], dirs [M,3], deltas [M,2], inv_s [1] (got {tuple(sdf.shape)}, "
                               f"{tuple(normals.shape)}, {tuple(dirs.shape)}, {tuple(deltas.shape)}, {tuple(inv_s.shape)})")
        sdf, normals, dirs, deltas, inv_s = (t.detach().to(dtype).contiguous() for t in tensors)
        sdf, inv_s = sdf.reshape(-1), inv_s.reshape(1)
        sigmas = torch.empty(n_samples, dtype=dtype, device=sdf.device)
        _geo.sdf_sigmas_forward(sdf, normals, dirs, deltas, inv_s, n_samples, cos_anneal, sigmas)
        ctx.save_for_backward(sdf, normals, dirs, deltas, inv_s)
        ctx.cos_anneal = float(cos_anneal)
        return sigmas

    @staticmethod
    def backward(ctx, grad_sigmas):
        if torch.is_grad_enabled() and grad_sigmas.requires_grad:
            raise RuntimeError("sdf_sigmas: second-order gradients are not provided (the op's backward is not differentiable; raymarching "
                               "stays first-order)")
        sdf, normals, dirs, deltas, inv_s = ctx.saved_tensors
        n_samples = sdf.shape[0]
        grad_sdf, grad_normals = torch.empty_like(sdf), torch.empty_like(normals)
        grad_dirs = torch.empty_like(dirs) if ctx.needs_input_grad[2] else None
        grad_inv_s = (torch.zeros_like if n_samples == 0 else torch.empty_like)(inv_s)   # without rows nothing is launched
        _geo.sdf_sigmas_backward(grad_sigmas.to(sdf.dtype).contiguous(), sdf, normals, dirs, deltas, inv_s, n_samples, ctx.cos_anneal, grad_sdf,
                                 grad_normals, grad_dirs, grad_inv_s)
        back = lambda g, like: None if g is None else g.view(like[0]).to(like[1])
        return (back(grad_sdf, ctx.like[0]), back(grad_normals, ctx.like[1]), back(grad_dirs, ctx.like[2]), None, back(grad_inv_s, ctx.like[4]),
                None)


def sdf_sigmas(sdf, normals, dirs, deltas, inv_s, cos_anneal=1.0):
    return _sdf_sigmas.apply(sdf, normals, dirs, deltas, inv_s, cos_anneal)


sdf_sigmas.__doc__ = _sdf_sigmas.__doc__


def surface_nets(volume, level, inside_below=False, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """extension (include/ngp_hip.h, ngp_surface_nets_count / _emit): the level set of volume [nz,ny,nx] (fp32, on the device)
    as an indexed triangle mesh by naive surface nets -> vertices [V,3] fp32 (x, y, z = fma(lattice, spacing, origin)), faces [F,3] int32,
    normals pointing from inside (above the level; inside_below: below it, as for an SDF) to outside.  Deterministic: the same bits on every
    run.  An export op: the two counts are read back between the two native calls.  An empty result is two zero-row tensors."""
    volume = volume.detach()
    ws = _geo.surface_nets_workspace(volume)
    counts = torch.empty(2, dtype=torch.int32, device=volume.device)
    _geo.surface_nets_count(volume, level, inside_below, ws, counts)
    n_vertices, n_faces = counts.tolist()
    if n_vertices < 0 or n_faces < 0:
        raise RuntimeError("surface_nets: the mesh does not fit int32 indices (more than 2^31 - 1 vertices or triangles)")
    vertices = torch.empty(n_vertices, 3, dtype=torch.float32, device=volume.device)
    faces = torch.empty(max(n_faces, 1), 3, dtype=torch.int32, device=volume.device)   # (the entry refuses a zero capacity)
    if n_vertices > 0:
        _geo.surface_nets_emit(volume, level, inside_below, origin, spacing, ws, vertices, faces)
    return vertices, faces[:n_faces]


def lattice_frame(lo, hi, dims):
    """the lattice of dims = (nx, ny, nz) points spanning [lo, hi] -> (origin, spacing), three Python floats each that are fp32 values:
    spacing = (hi - lo) / (N - 1) computed in double and narrowed ONCE -- the `origin` / `spacing` of surface_nets over a volume filled on it"""
    def triple(v):
        return [float(x) for x in v] if hasattr(v, '__len__') else [float(v)] * 3

    def narrow(x):
        return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))
    lo, hi, dims = triple(lo), triple(hi), [int(n) for n in dims]
    if len(dims) != 3 or min(dims) < 1:
        raise RuntimeError(f"lattice: dims must be (nx, ny, nz), each at least 1 (got {dims})")
    return [narrow(a) for a in lo], [narrow((b - a) / (n - 1)) if n > 1 else 0.0 for a, b, n in zip(lo, hi, dims)]


def lattice_points(lo, hi, dims, z0, z1, bitfield=None, bound=1, cascade=1, grid_size=128, dilate=1, device=None):
    """extension (ngp_lattice_points): the points of the z-slab [z0, z1) of the lattice dims = (nx, ny, nz) over [lo, hi] that
    lie near occupied space -- one of the (2 dilate + 1)^3 cells of `bitfield` around the point's own cell, at the cascade the marcher would
    look it up in, is set -- compacted in lattice order -> points [K,3] fp32, index [K] int32 (the linear index (k ny + j) nx + i in the whole
    lattice).  bitfield None: every point of the slab.  One read-back (K)."""
    nx, ny, nz = (int(n) for n in dims)
    if not 0 <= z0 < z1 <= nz:
        raise RuntimeError(f"lattice_points: the slab [{z0}, {z1}) must be a non-empty range of [0, {nz})")
    if bitfield is not None:
        device = bitfield.device
    elif device is None:
        device = torch.device('cuda')
    origin, spacing = lattice_frame(lo, hi, dims)
    capacity = nx * ny * (z1 - z0)
    points = torch.empty(capacity, 3, dtype=torch.float32, device=device)
    index = torch.empty(capacity, dtype=torch.int32, device=device)
    count = torch.empty(1, dtype=torch.int32, device=device)
    _geo.lattice_points(origin, spacing, nx, ny, z0, z1, bitfield, bound, cascade, grid_size, dilate, points, index, count)
    kept = int(count.item())
    return points[:kept], index[:kept]


def _ray_dtype(*tensors):
    """float64 when one of the floating tensors is, else float32 (the rule of the compositors' float64 twins)"""
    return torch.float64 if any(t is not None and t.dtype == torch.float64 for t in tensors) else torch.float32


def sample_ts(xyzs, rays_o, rays_d, rays, bound):
    """Extension (not in the reference): ts [M], the t of every sample of march_rays_train's xyzs [M,3] along its ray,
    recovered from the marcher's output (which keeps t to itself): t = sum_j m_j d_j (x_j - o_j) / sum_j m_j d_j^2 over the coordinates that
    were not clamped to +-bound.  Rows no ray owns are 0.  No autograd: the sample parameters are constants of the pose."""
    dtype = _ray_dtype(xyzs, rays_o, rays_d)
    xyzs = xyzs.detach().to(dtype).contiguous()
    rays_o, rays_d = _rays(rays_o.detach().to(dtype)), _rays(rays_d.detach().to(dtype))
    ts = torch.empty(xyzs.shape[0], dtype=dtype, device=xyzs.device)
    _geo.ray_sample_ts(xyzs, rays_o, rays_d, rays.contiguous(), xyzs.shape[0], rays.shape[0], bound, ts)
    return ts


class _ray_points(Function):
    """Extension (not in the reference): the samples of the training rays as a differentiable function of the rays,
    x_i = clamp(o_n + t_i d_n, -bound, bound) and dirs_i = d_n with the marcher's t_i as constants.  A clamped coordinate passes no gradient.
    First order only."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, ts, rays, bound, like_xyzs, like_dirs):
        dtype = _ray_dtype(rays_o, rays_d, ts, like_xyzs)
        ctx.shapes = (rays_o.shape, rays_d.shape, rays_o.dtype, rays_d.dtype)
        rays_o, rays_d = _rays(rays_o.to(dtype)), _rays(rays_d.to(dtype))
        ts, rays = ts.to(dtype).contiguous(), rays.contiguous()
        n_samples, n_rays = ts.shape[0], rays.shape[0]
        if like_xyzs is not None:   # the marcher's own tensors: a render's forward does not change by a bit
            xyzs, dirs = like_xyzs, like_dirs
            if xyzs.dtype != dtype or tuple(xyzs.shape) != (n_samples, 3) or tuple(dirs.shape) != (n_samples, 3):
                raise RuntimeError(f"ray_points: like=(xyzs, dirs) must be two [{n_samples}, 3] {dtype} tensors (got {tuple(xyzs.shape)} "
                                   f"{xyzs.dtype}, {tuple(dirs.shape)} {dirs.dtype})")
        else:
            xyzs = torch.empty(n_samples, 3, dtype=dtype, device=ts.device)
            dirs = torch.empty_like(xyzs)
            _geo.ray_points_forward(rays_o, rays_d, ts, rays, n_samples, n_rays, bound, xyzs, dirs)
        ctx.save_for_backward(xyzs.detach().contiguous(), ts, rays_d, rays)
        ctx.bound = bound
        ctx.set_materialize_grads(False)
        return xyzs, dirs

    @staticmethod
    def backward(ctx, grad_xyzs, grad_dirs):
        if torch.is_grad_enabled() and any(g is not None and g.requires_grad for g in (grad_xyzs, grad_dirs)):
            raise RuntimeError("ray_points: second-order gradients are not provided (raymarching stays first-order)")
        xyzs, ts, rays_d, rays = ctx.saved_tensors
        shape_o, shape_d, dtype_o, dtype_d = ctx.shapes
        n_samples, n_rays = ts.shape[0], rays.shape[0]
        dense = lambda g: None if g is None else g.to(ts.dtype).contiguous()
        grad_xyzs = torch.zeros_like(xyzs) if grad_xyzs is None else dense(grad_xyzs)
        grad_rays_o = torch.empty(n_rays, 3, dtype=ts.dtype, device=ts.device)
        grad_rays_d = torch.empty_like(grad_rays_o)
        _geo.ray_points_backward(grad_xyzs, dense(grad_dirs), None, xyzs, ts, rays_d, rays, n_samples, n_rays, ctx.bound, grad_rays_o, grad_rays_d)
        return grad_rays_o.view(shape_o).to(dtype_o), grad_rays_d.view(shape_d).to(dtype_d), None, None, None, None, None


def ray_points(rays_o, rays_d, ts, rays, bound, like=None):
    """rays_o / rays_d [N,3], ts [M] (sample_ts), rays [N,3] int32 (march_rays_train) -> xyzs [M,3], dirs [M,3], differentiable in rays_o
    and rays_d (float32 or float64).  like=(xyzs, dirs): return the marcher's own tensors (unchanged bits) with this op's backward -- the
    form the renderer uses; without it both are computed (ngp_ray_points_forward: clamp(fma(t, d, o)), rows no ray owns are zero)."""
    like_xyzs, like_dirs = (None, None) if like is None else like
    return _ray_points.apply(rays_o, rays_d, ts, rays, bound, like_xyzs, like_dirs)


# ----------------------------------------------------------------------------------------------
# inference
# ----------------------------------------------------------------------------------------------
class _march_rays(Function):
    @staticmethod
    @_f32_fwd
    def forward(ctx, n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, density_bitfield, C, H, near, far, align=-1,
                perturb=False, dt_gamma=0, max_steps=1024):
        """advance every alive ray by up to n_step occupied samples -> xyzs, dirs [n_alive*n_step (padded), 3], deltas [.., 2];
        unused slots stay zero (deltas == 0 marks "ray finished" for composite_rays)"""
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        dev = rays_o.device
        slots = _round_up_strict(n_alive * n_step, align)
        # the kernel zeroes every slot it does not fill (ngp_march_rays_ex): no memsets, no noise tensor unless perturbing
        xyzs = torch.empty(slots, 3, dtype=torch.float32, device=dev)
        dirs = torch.empty(slots, 3, dtype=torch.float32, device=dev)
        deltas = torch.empty(slots, 2, dtype=torch.float32, device=dev)
        noises = torch.rand(n_alive, dtype=torch.float32, device=dev) if perturb else None
        _backend.march_rays_ex(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H,
                               density_bitfield.contiguous(), near, far, xyzs, dirs, deltas, noises, slots)
        return xyzs, dirs, deltas


march_rays = _march_rays.apply


class _composite_rays(Function):
    @staticmethod
    @_f32_fwd
    def forward(ctx, n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, T_thresh=1e-2):
        """accumulate in place into weights_sum/depth/image [N]; rays_alive[i] = -1 when the ray stopped early, else rays_t advances"""
        _backend.composite_rays(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas.contiguous(), rgbs.contiguous(),
                                deltas.contiguous(), weights_sum, depth, image)
        return tuple()


composite_rays = _composite_rays.apply


def composite_rays_features(n_alive, n_step, rays_alive, sigmas, feats, deltas, weights_sum, out, T_thresh=1e-2):
    """Extension (not in the reference): the caller's per-sample channels in the inference loop.  out [N,C] float32 is updated
    in place, out[rays_alive[n], c] += sum of w * feats[n * n_step + step, c] over the samples composite_rays composites for list entry n,
    with that op's weights (the same statements: with feats = rgbs the bits of its image, with a channel of ones those of weights_sum).
    CALL ORDER: before composite_rays of the same rows -- it reads the weights_sum that call advances, and changes nothing but `out`
    (rays_alive, rays_t, weights_sum stay as they are).  No background is blended in.
    feats [>= n_alive * n_step, C], contiguous, float32 or float16, 1 <= C <= 256: float16 stays float16 (also under autocast; converted at the
    load, accumulated in float32).  sigmas / deltas / weights_sum are taken as float32.  float64 is not provided.  No autograd: feats is
    detached.  Rows at or behind a ray's end (deltas == 0, or behind the sample that crosses T_thresh) are not read."""
    for t, name in ((sigmas, 'sigmas'), (feats, 'feats'), (deltas, 'deltas'), (weights_sum, 'weights_sum'), (out, 'out')):
        if t.dtype == torch.float64:
            raise TypeError(f"composite_rays_features: {name} is float64; the inference feature compositor takes float32 (feats: float32 or float16)")
    feats = feats.detach()
    if feats.dtype != torch.float16:  # no custom_fwd cast: it would up-cast float16 features
        feats = feats.float()
    if feats.dim() != 2 or out.dim() != 2 or feats.shape[1] != out.shape[1] or feats.shape[0] < n_alive * n_step:
        raise RuntimeError(f"composite_rays_features: feats must be [>= {n_alive * n_step}, C] and out [N, C] (got {tuple(feats.shape)}, "
                           f"{tuple(out.shape)})")
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("composite_rays_features: out must be a contiguous float32 tensor (it is updated in place)")
    _geo.composite_rays_features(n_alive, n_step, T_thresh, rays_alive, sigmas.detach().float().contiguous(), feats.contiguous(),
                                 deltas.detach().float().contiguous(), weights_sum.detach().float().contiguous(), out)
    return out


def compact_rays(rays_alive, n_alive=None):
    """Extension: order-preserving device-side equivalent of `rays_alive[rays_alive >= 0]`.
    Returns (compacted [n_alive] int32 -- only the first count entries are meaningful, count [1] int32 on device)."""
    n_alive = rays_alive.shape[0] if n_alive is None else n_alive
    out = torch.empty(max(n_alive, 1), dtype=torch.int32, device=rays_alive.device)
    count = torch.zeros(1, dtype=torch.int32, device=rays_alive.device)
    _backend.compact_rays(rays_alive, n_alive, out, count)
    return out, count
