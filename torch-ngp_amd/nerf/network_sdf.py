"""A NeuS-style signed-distance model on the library's own blocks (extension), in the style of network_ff.py:
hash grid -> FFMLP(32 -> 64 -> 16), output 0 + an analytic sphere prior |x| - r0 = the SDF, outputs 1..15 = features;
SH(3) direction code (9) ++ normal (3) ++ features (15) ++ 5 zero pads (= 32) -> FFMLP(32 -> 64 -> 3) -> sigmoid = the colour.
The normal is the SDF's gradient, autograd.grad(sdf, x, create_graph=training): the second-order backwards of the grid encoder and the
FFMLP carry a loss on it -- through the colour, through raymarching.sdf_sigmas, or an eikonal term -- to the table and
the weights.  forward(x, d, deltas) turns the SDF into the density the compositors render with raymarching.sdf_sigmas (NeuS's section
opacity), so render(), geo=True, aux= and aux_infer= work as for a density model.

The FFMLP has no bias: the sphere prior gives a valid surface and |grad f| ~ 1 at initialisation.  Like network_ff.py the model is meant to
run under fp16 autocast (the FFMLP kernels take half tensors)."""
import math

import torch
import torch.nn as nn

import raymarching
from encoding import get_encoder
from ffmlp import FFMLP
from ffmlp.ffmlp import ffmlp_forward

from .renderer import NeRFRenderer


class NeuSNetwork(NeRFRenderer):
    # the renderer hands the marcher's deltas to forward (run_cuda, render_loop.StageIssuer); the eval loop runs stage by stage, eagerly
    takes_deltas = True
    graph_loop = False
    native_loop = False

    def __init__(self, hidden_dim=64, geo_feat_dim=15, hidden_dim_color=64, bound=1, log2_hashmap_size=19, prior_radius=0.5, init_inv_s=20.0,
                 cos_anneal=1.0, deterministic=None, **kwargs):
        super().__init__(bound, **kwargs)
        self.geo_feat_dim = geo_feat_dim
        self.prior_radius = float(prior_radius)
        self.cos_anneal = float(cos_anneal)   # host attribute, NeuS's cos_anneal_ratio in [0, 1]: the trainer raises it from 0 to 1
        self.encoder, self.in_dim = get_encoder('hashgrid', desired_resolution=2048 * bound, log2_hashmap_size=log2_hashmap_size)
        self.encoder.deterministic = deterministic
        self.sdf_net = FFMLP(input_dim=self.in_dim, output_dim=1 + geo_feat_dim, hidden_dim=hidden_dim, num_layers=2, activation='softplus')
        self.encoder_dir, dir_dim = get_encoder('sphere_harmonics', degree=3)
        self.pad_color = 32 - (dir_dim + 3 + geo_feat_dim)
        assert self.pad_color >= 0, 'SH code + normal + features must fit the 32 inputs of the colour network'
        self.color_net = FFMLP(input_dim=32, output_dim=3, hidden_dim=hidden_dim_color, num_layers=2)
        self.log_inv_s = nn.Parameter(torch.full((1,), math.log(init_inv_s)))   # NeuS's learnable sharpness, inv_s = exp(log_inv_s)
        self.last_normals = None   # the normals of the last forward [M,3]: what an aux= / aux_infer= callable composites as a normal map

    @property
    def inv_s(self):
        return torch.exp(self.log_inv_s.float())

    def _sdf_head(self, x, differentiable):
        """-> sdf [M] fp32, features [M,15].  differentiable: through the FFMLP's training kernel whatever the mode (the inference kernel
        keeps nothing for a backward, and the normal is a backward)"""
        enc = self.encoder(x, bound=self.bound)
        if differentiable:
            net, pad = self.sdf_net, 128 - (enc.shape[0] % 128)
            padded = torch.cat([enc, torch.zeros(pad, enc.shape[1], dtype=enc.dtype, device=enc.device)], dim=0)
            h = ffmlp_forward(padded, net.weights, net.input_dim, net.padded_output_dim, net.hidden_dim, net.num_layers, net.activation,
                              net.output_activation, False, True)[:enc.shape[0], :net.output_dim]
        else:
            h = self.sdf_net(enc)
        prior = torch.sqrt((x.float() ** 2).sum(-1) + 1e-12) - self.prior_radius
        return h[..., 0].float() + prior, h[..., 1:]

    def sdf_and_normal(self, x, with_features=False):
        """x [M,3] -> sdf [M], normal [M,3] = d sdf / d x (not normalised).  Training: both stay in the graph (create_graph), for eikonal
        terms on points of the caller's choosing; eval: detached, computed under a local enable_grad (also inside a frame's no_grad)."""
        with torch.enable_grad():
            if not x.requires_grad:
                x = x.detach().requires_grad_(True)
            sdf, feat = self._sdf_head(x, True)
            normals = torch.autograd.grad(sdf.sum(), x, create_graph=self.training)[0]
        if not self.training:
            sdf, normals, feat = sdf.detach(), normals.detach(), feat.detach()
        return (sdf, normals, feat) if with_features else (sdf, normals)

    def _color_head(self, d, normals, feat):
        code = self.encoder_dir(d)
        pad = torch.zeros(code.shape[0], self.pad_color, dtype=code.dtype, device=code.device)
        return torch.sigmoid(self.color_net(torch.cat([code, normals.to(code.dtype), feat.to(code.dtype), pad], dim=-1)))

    def forward(self, x, d, deltas=None):
        # x [M,3] in [-bound, bound], d [M,3] unit directions, deltas [M,2] (the marcher's) -> sigma [M], rgb [M,3]
        if deltas is None:
            raise ValueError("NeuSNetwork.forward needs the marcher's deltas (the opacity of an SDF sample depends on the section length); "
                             "the renderer passes them to a model with takes_deltas")
        sdf, normals, feat = self.sdf_and_normal(x, with_features=True)
        self.last_normals = normals
        sigmas = raymarching.sdf_sigmas(sdf, normals, d, deltas, self.inv_s, self.cos_anneal)
        return sigmas, self._color_head(d, normals, feat)

    def density(self, x):
        """{'sigma': inv_s (1 - sigmoid(inv_s f))} for the occupancy refresh: the direction-free bound of NeuS's continuous opaque density
        inv_s (1 - Phi) |cos| |grad f| at |grad f| = 1.  No gradient is needed (and none is computed: the SDF alone, no normal)."""
        with torch.no_grad():
            sdf, _ = self._sdf_head(x, False)
            inv_s = self.inv_s
            return {'sigma': inv_s * torch.sigmoid(-inv_s * sdf)}

    # extract_mesh contours the SDF itself (not the density the occupancy refresh sees): level 0, inside below it, and a lattice point the
    # occupancy cull skipped counts as outside (+1)
    mesh_level, mesh_inside_below, mesh_fill = 0.0, True, 1.0

    def _mesh_values(self, pts):
        return self._sdf_head(pts, False)[0].float()

    def extract_mesh(self, *args, normals=False, **kwargs):
        """NeRFRenderer.extract_mesh on the SDF; normals=True appends the unit normals at the vertices [V,3] (the SDF's gradient through
        sdf_and_normal, normalised)"""
        out = super().extract_mesh(*args, **kwargs)
        if not normals:
            return out
        was_training = self.training
        self.eval()
        try:
            with torch.autocast('cuda', dtype=torch.float16, enabled=out[0].is_cuda):
                n = torch.cat([self.sdf_and_normal(part)[1].float() for part in out[0].split(1 << 20)]) if out[0].shape[0] else out[0].clone()
        finally:
            self.train(was_training)
        return (*out, torch.nn.functional.normalize(n, dim=-1))

    def get_params(self, lr):
        groups = [{'params': m.parameters(), 'lr': lr} for m in (self.encoder, self.sdf_net, self.encoder_dir, self.color_net)]
        return groups + [{'params': [self.log_inv_s], 'lr': lr}]
