"""Ray generation of the data path: `get_rays(poses, intrinsics, H, W, N=-1, error_map=None, patch_size=1)` with the argument
meaning and the result dictionary of the reference (nerf/utils.py:53-137: 'rays_o', 'rays_d' [B,N,3], 'inds' [B,N] when N > 0,
'inds_coarse' with an error map).  Which pixels are drawn is decided with the same torch calls as there (uniform with replacement,
patch corners, or a multinomial draw on the 128 x 128 error map refined by a uniform offset); turning pixels into rays -- pinhole
direction, normalisation, camera-to-world rotation, origin broadcast: eight elementwise/bmm launches in the reference -- is one HIP
kernel (ngp_rays_from_pixels) that writes the [B,N,3] outputs directly, optionally into caller-provided buffers (`out=`), e.g. the static
input buffers of graph.GraphedTrainStep.

Error-map sampling on the device (extension): `get_rays(..., error_map=, seed=)` draws the pixels with ngp_error_map_draw --
the same weighted draw without replacement, one launch, no torch generator -- and `ErrorMaps` keeps the per-image maps and applies the
Trainer's EMA update (ngp_error_map_update).  `seed=None` is the torch path above, unchanged.

SURVEY.md 8(f).4.  Fails loudly without the HIP library: there is no CPU fallback."""
import torch

import _ngp_capi as capi


def custom_meshgrid(*args):
    return torch.meshgrid(*args, indexing='ij')


def _draw_pixels(B, H, W, N, error_map, patch_size, device):
    """-> (inds [B,N] or [N] int64, inds_coarse or None); the three sampling modes of the reference, same distributions"""
    if patch_size > 1:  # square patches from random top-left corners (the error map is ignored, as in the reference)
        n_patches = N // (patch_size ** 2)
        top = torch.randint(0, H - patch_size, size=[n_patches], device=device)
        left = torch.randint(0, W - patch_size, size=[n_patches], device=device)
        dy, dx = custom_meshgrid(torch.arange(patch_size, device=device), torch.arange(patch_size, device=device))
        rows = top[:, None] + dy.reshape(1, -1)
        cols = left[:, None] + dx.reshape(1, -1)
        return (rows * W + cols).reshape(-1), None
    if error_map is None:
        return torch.randint(0, H * W, size=[N], device=device), None
    coarse = torch.multinomial(error_map.to(device), N, replacement=False)  # [B,N] cells of the 128 x 128 map
    cell_h, cell_w = H / 128, W / 128
    rows = ((coarse // 128) * cell_h + torch.rand(B, N, device=device) * cell_h).long().clamp(max=H - 1)
    cols = ((coarse % 128) * cell_w + torch.rand(B, N, device=device) * cell_w).long().clamp(max=W - 1)
    return rows * W + cols, coarse


def _seed_words(seed):
    """(host word, device word or None) of a `seed=` argument: a Python int, or a one-word CUDA tensor the kernel reads itself (int32, e.g.
    optimizer.scalars[STEP_COUNT:STEP_COUNT + 1] -- the word `noise_seed` uses; any 4-byte dtype: the bits are the seed)"""
    if torch.is_tensor(seed):
        if not (seed.is_cuda and seed.numel() == 1 and seed.element_size() == 4):
            raise RuntimeError('error-map draw: a tensor seed must be a one-element 4-byte CUDA tensor (int32)')
        return 0, seed
    return int(seed) & 0xffffffff, None


def draw_error_map(error_map, H, W, N, seed, res=128, keys_out=None, n_drawable=None):
    """Extension: N distinct cells per image of error_map [B, res * res] (fp32, CUDA), drawn without replacement proportional
    to the map, refined to pixels of the H x W frame -- ngp_error_map_draw: one launch, no torch generator, the same outputs for the same
    (map, seed).  -> (inds [B,N], inds_coarse [B,N]) int64, ascending cell order.  keys_out [B, res * res] fp32 / n_drawable [B] int32:
    optional tensors that receive every cell's race key / the number of cells with a finite positive weight."""
    if not error_map.is_cuda:
        raise RuntimeError('error-map draw: error_map must be a CUDA tensor (the MI355X build has no CPU path)')
    if error_map.dim() != 2 or error_map.shape[1] != res * res:
        raise RuntimeError(f'error-map draw: error_map must be [B, {res * res}] for res={res} (got {tuple(error_map.shape)})')
    em = error_map.float().contiguous()
    B = em.shape[0]
    word, word_dev = _seed_words(seed)
    inds = torch.empty(B, N, dtype=torch.int64, device=em.device)
    coarse = torch.empty(B, N, dtype=torch.int64, device=em.device)
    capi.check(capi.lib.ngp_error_map_draw(em.data_ptr(), B, int(res), int(N), int(H), int(W), word, capi.ptr(word_dev), inds.data_ptr(),
                                           coarse.data_ptr(), capi.ptr(keys_out), capi.ptr(n_drawable), capi.stream()))
    return inds, coarse


class ErrorMaps:
    """Extension: the per-image error maps of the reference's `--error_map` training (provider.py: torch.ones([n_images,
    128 * 128]); Trainer.train_step: 0.1 / 0.9 EMA of the per-ray squared error at the drawn cells), kept on the device and served by the
    two kernels of csrc/error_map.hip.  `.maps` [n_images, res * res] fp32 is a plain tensor: save and load it as one.

        inds, coarse = maps.draw(i, H, W, N, seed)                    # or get_rays(..., error_map=maps.maps[i:i + 1], seed=seed)
        ... get_rays(out=...) / pose_rays, stepper.step(...) ...
        maps.update(i, coarse, stepper.image, target)

    With GraphedTrainStep.step(next_rays=) the following batch is drawn before this update: it sees a map that is one step stale."""

    def __init__(self, n_images, device, res=128):
        if not 1 <= int(res) <= 128:
            raise ValueError('ErrorMaps: res must be in [1, 128]')
        self.res = int(res)
        self.maps = torch.ones(int(n_images), self.res * self.res, dtype=torch.float32, device=device)

    def draw(self, index, H, W, N, seed):
        """-> (inds [1,N], inds_coarse [1,N]) int64 for image `index`"""
        return draw_error_map(self.maps[index:index + 1], H, W, N, seed, res=self.res)

    @torch.no_grad()
    def update(self, index, inds_coarse, image, target, keep=0.1, take=0.9):
        """maps[index, c] = keep * maps[index, c] + take * mean_k (image - target)^2 at the rays' cells c = inds_coarse, in place (one launch);
        image, target [N,3] fp32 (e.g. GraphedTrainStep.image and the step's target)"""
        row = self.maps[index]
        n = inds_coarse.numel()
        for t, name in ((image, 'image'), (target, 'target')):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 3 * n):
                raise RuntimeError(f'ErrorMaps.update: {name} must be a contiguous float32 CUDA tensor of N*3 elements')
        if not (inds_coarse.is_cuda and inds_coarse.dtype == torch.int64 and inds_coarse.is_contiguous()):
            raise RuntimeError('ErrorMaps.update: inds_coarse must be a contiguous int64 CUDA tensor')
        capi.check(capi.lib.ngp_error_map_update(row.data_ptr(), inds_coarse.data_ptr(), image.data_ptr(), target.data_ptr(), n, row.numel(),
                                                 float(keep), float(take), capi.stream()))


@torch.no_grad()
def get_rays(poses, intrinsics, H, W, N=-1, error_map=None, patch_size=1, out=None, seed=None, res=128):
    """poses [B,4,4] cam2world (CUDA, fp32), intrinsics (fx, fy, cx, cy).  `out=(rays_o, rays_d)`: optional contiguous fp32 [B,n,3]
    tensors to fill (extension).  `seed=` (extension; with an error_map and patch_size 1): a Python int or a one-word int32 CUDA tensor --
    the pixels come from ngp_error_map_draw (draw_error_map above: no torch generator, `res` x `res` map) instead of torch.multinomial;
    None keeps the torch path."""
    if not poses.is_cuda:
        raise RuntimeError('get_rays: poses must be a CUDA tensor (the MI355X build has no CPU path)')
    poses = poses.float().contiguous()
    B = poses.shape[0]
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    results = {}
    if N > 0:
        N = min(N, H * W)
        if seed is not None and error_map is not None and patch_size <= 1:
            inds, coarse = draw_error_map(error_map.to(poses.device), H, W, N, seed, res=res)
        else:
            inds, coarse = _draw_pixels(B, H, W, N, error_map, patch_size, poses.device)
        n = inds.shape[-1]
        shared = inds.dim() == 1
        inds = inds.contiguous()
        results['inds'] = inds.expand(B, n) if shared else inds
        if coarse is not None:
            results['inds_coarse'] = coarse
        inds_ptr, stride = inds.data_ptr(), (0 if shared else n)
    else:
        n, inds_ptr, stride = H * W, None, 0
    if out is None:
        rays_o = torch.empty(B, n, 3, device=poses.device, dtype=torch.float32)
        rays_d = torch.empty(B, n, 3, device=poses.device, dtype=torch.float32)
    else:
        rays_o, rays_d = out
        for t in (rays_o, rays_d):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == B * n * 3):
                raise RuntimeError('get_rays: out tensors must be contiguous float32 CUDA tensors of B*N*3 elements')
    capi.check(capi.lib.ngp_rays_from_pixels(poses.data_ptr(), B, fx, fy, cx, cy, W, inds_ptr, stride, n, rays_o.data_ptr(), rays_d.data_ptr(),
                                             capi.stream()))
    results['rays_o'] = rays_o.view(B, n, 3)
    results['rays_d'] = rays_d.view(B, n, 3)
    return results


class _pose_rays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses, fx, fy, cx, cy, W, inds, n):
        B = poses.shape[0]
        dtype_in = poses.dtype
        poses = poses.float().contiguous()
        rays_o = torch.empty(B, n, 3, device=poses.device, dtype=torch.float32)
        rays_d = torch.empty_like(rays_o)
        inds_ptr, stride = (None, 0) if inds is None else (inds.data_ptr(), 0 if inds.dim() == 1 else n)
        capi.check(capi.lib.ngp_rays_from_pixels(poses.data_ptr(), B, fx, fy, cx, cy, W, inds_ptr, stride, n, rays_o.data_ptr(), rays_d.data_ptr(),
                                                 capi.stream()))
        ctx.args = (B, fx, fy, cx, cy, W, inds, stride, n, dtype_in)
        ctx.set_materialize_grads(False)
        return rays_o, rays_d

    @staticmethod
    def backward(ctx, grad_o, grad_d):
        if torch.is_grad_enabled() and any(g is not None and g.requires_grad for g in (grad_o, grad_d)):
            raise RuntimeError('pose_rays: second-order gradients are not provided')
        B, fx, fy, cx, cy, W, inds, stride, n, dtype_in = ctx.args
        ref = grad_o if grad_o is not None else grad_d
        dense = lambda g: torch.zeros(B, n, 3, device=ref.device, dtype=torch.float32) if g is None else g.float().contiguous()
        grad_o, grad_d = dense(grad_o), dense(grad_d)
        grad_poses = torch.empty(B, 4, 4, device=ref.device, dtype=torch.float32)
        capi.check(capi.lib.ngp_rays_from_pixels_backward(grad_o.data_ptr(), grad_d.data_ptr(), B, fx, fy, cx, cy, W, capi.ptr(inds), stride, n,
                                                          grad_poses.data_ptr(), capi.stream()))
        return grad_poses.to(dtype_in), None, None, None, None, None, None, None


def pose_rays(poses, intrinsics, H, W, inds=None):
    """Extension (not in the reference): the rays of given pixels as a differentiable function of the camera poses.
    poses [B,4,4] cam2world (CUDA), intrinsics (fx, fy, cx, cy), inds: int64 pixel indices [n] (shared by the poses) or [B,n], None = the full
    H x W frame -> rays_o, rays_d [B,n,3] with the bits of get_rays for the same pixels (the same kernel); the backward is
    ngp_rays_from_pixels_backward.  get_rays itself stays as it is (no_grad).  A pose parametrisation (e.g. poses = exp(xi) @ poses0) is
    built in torch on top of this."""
    if not poses.is_cuda:
        raise RuntimeError('pose_rays: poses must be a CUDA tensor (the MI355X build has no CPU path)')
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    if inds is not None:
        if inds.dtype != torch.int64 or inds.dim() not in (1, 2) or (inds.dim() == 2 and inds.shape[0] != poses.shape[0]):
            raise RuntimeError('pose_rays: inds must be an int64 tensor of shape [n] or [B,n]')
        inds = inds.to(poses.device).contiguous()
    n = H * W if inds is None else inds.shape[-1]
    return _pose_rays.apply(poses, fx, fy, cx, cy, int(W), inds, n)


def save_mesh(path, vertices, faces, normals=None):
    """write an indexed triangle mesh as a binary little-endian PLY with numpy alone (the reference's save_mesh needs trimesh): vertices
    [V,3] float32 (x, y, z), optional normals [V,3] float32 (nx, ny, nz), faces [F,3] int32 as `list uchar int vertex_indices`.  Tensors
    (any device) or arrays."""
    import numpy as np

    def host(a, dtype, what):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"save_mesh: {what} must be [n,3] (got {a.shape})")
        return np.ascontiguousarray(a, dtype)
    v, f = host(vertices, '<f4', 'vertices'), host(faces, '<i4', 'faces')
    names = ['x', 'y', 'z']
    if normals is not None:
        n = host(normals, '<f4', 'normals')
        if len(n) != len(v):
            raise ValueError(f"save_mesh: {len(n)} normals for {len(v)} vertices")
        v, names = np.concatenate([v, n], axis=1), names + ['nx', 'ny', 'nz']
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("save_mesh: a face names a vertex that does not exist")
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}'] + [f'property float {n}' for n in names] + \
             [f'element face {len(f)}', 'property list uchar int vertex_indices', 'end_header']
    rows = np.empty(len(f), dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    rows['n'], rows['v'] = 3, f
    with open(path, 'wb') as out:
        out.write(('\n'.join(header) + '\n').encode('ascii'))
        out.write(v.tobytes())
        out.write(rows.tobytes())
