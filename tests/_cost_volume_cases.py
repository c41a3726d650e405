"""The cases of tests/test_cost_volume_bwd_gpu.py: inputs drawn on the CPU from a seed, and the conditions on them that the float64
reference alone decides (tests/test_stage_f64_cpu.py checks those without a GPU, so a seed can be chosen on any machine)."""
import torch

from _stage_f64 import clear_of_zero, cost_volume_f64
from _util import reference_state_dict

BAND = 2e-6          # the forward's bound (tests/test_stage_f64_gpu.py::_check): an activation this close to zero, relative to its layer's
                     # largest magnitude, may take either slope
PARAMS = ["wd", "w2", "b2", "w3", "b3", "wa", "ba", "wb", "bb", "wc", "bc"]

# (id, B, n1, n2, seed, live): what each enters is in the table of test_cost_volume_bwd_gpu.py
CASES = [
    ("b3_n77", 3, 77, 77, 1, None),
    ("b2_n50_from_131", 2, 50, 131, 2, None),
    ("b2_n131_from_50", 2, 131, 50, 3, None),
    ("b5_n1_from_16", 5, 1, 16, 4, None),
    ("b64_n37_looping", 64, 37, 37, 5, None),
    ("b100_n22_from_16_looping", 100, 22, 16, 6, None),
    ("b3_n77_padded", 3, 77, 77, 7, (40, 77, 17)),
]
LOOPING = {"b64_n37_looping", "b100_n22_from_16_looping"}


def case_by_name(name):
    return Case(*next(c for c in CASES if c[0] == name))


def parameters(device, dtype):
    """[wd, w2, b2, w3, b3, wa, ba, wb, bb, wc, bc] of the reference state dict's fc_layer, split as train_path.correlator_train
    splits them: wd = the direction columns of conv 0 (after the two 256-channel feature segments), convs 1 and 2, weightnet1."""
    sd = reference_state_dict("cpu")
    w0 = sd["fc_layer.mlp_convs.0.weight"].flatten(1)
    out = [w0[:, w0.shape[1] - 3:]]
    for i in (1, 2):
        out += [sd["fc_layer.mlp_convs.%d.weight" % i].flatten(1), sd["fc_layer.mlp_convs.%d.bias" % i]]
    for i in range(3):
        out += [sd["fc_layer.weightnet1.mlp_convs.%d.weight" % i].flatten(1), sd["fc_layer.weightnet1.mlp_convs.%d.bias" % i]]
    return [t.to(device=device, dtype=dtype).contiguous() for t in out]


class Case:
    """Clouds of unit size xyz1 (B, n1, 3), xyz2 (B, n2, 3) -- where n2 <= n1 a perturbed copy of xyz1's first n2 points --, p1
    (B n1, 256), p2 (B n2, 256) and the cotangent ct (B n1, 256), drawn on the CPU.  live (B,): the queries and the points from live[b]
    on are copies of query / point 0, coordinates and rows (a padded batch); they are no kNN candidates."""

    def __init__(self, name, B, n1, n2, seed, live=None):
        g = torch.Generator().manual_seed(seed)
        self.name, self.B, self.n1, self.n2, self.live = name, B, n1, n2, live
        xyz1 = torch.randn(B, n1, 3, generator=g)
        xyz2 = torch.randn(B, n2, 3, generator=g)
        if n2 <= n1:
            xyz2 = xyz1[:, :n2] + 0.3 * xyz2
        p1, p2 = torch.randn(B, n1, 256, generator=g), torch.randn(B, n2, 256, generator=g)
        if live is not None:
            assert len(live) == B and all(16 <= v <= min(n1, n2) for v in live)
            for b, v in enumerate(live):
                xyz1[b, v:], xyz2[b, v:], p1[b, v:], p2[b, v:] = xyz1[b, 0], xyz2[b, 0], p1[b, 0], p2[b, 0]
        self.xyz1, self.xyz2 = xyz1.contiguous(), xyz2.contiguous()
        self.p1, self.p2 = p1.reshape(B * n1, 256).contiguous(), p2.reshape(B * n2, 256).contiguous()
        self.ct = torch.randn(B * n1, 256, generator=g)

    def knn_host(self):
        """The neighbour table by torch on the host (choosing a seed without a GPU; the GPU tests take the kernels' tables)."""
        x1, x2 = self.xyz1.double(), self.xyz2.double()
        d = ((x1[:, :, None, :] - x2[:, None, :, :]) ** 2).sum(-1)
        if self.live is not None:
            cand = torch.arange(self.n2)[None, :] >= torch.tensor(self.live)[:, None]
            d = d.masked_fill(cand[:, None, :], float("inf"))
        return d.topk(16, dim=2, largest=False).indices

    def reference(self, knn, par, dtype, device, decisions=None, ct=None, grads=True):
        """cost_volume_f64 in `dtype` on `device` -> (out (B n1, 256), [a1, a2, a3] each (B n1 16, 256), the 13 gradients under the
        cotangent `ct` in the operator's order p1, p2, PARAMS; None without `grads`).  par: the 11 parameters in any dtype."""
        B, n1, n2 = self.B, self.n1, self.n2
        c = lambda t: t.detach().to(device=device, dtype=dtype)
        leaves = [c(self.p1).view(B, n1, 256), c(self.p2).view(B, n2, 256)] + [c(t) for t in par]
        if grads:
            leaves = [t.requires_grad_(True) for t in leaves]
        p1, p2, wd, w2, b2, w3, b3, wa, ba, wb, bb, wc, bc = leaves
        with torch.set_grad_enabled(grads):
            out, acts = cost_volume_f64(c(self.xyz1), c(self.xyz2), knn.to(device), p1, p2, wd, [(w2, b2), (w3, b3)],
                                        [(wa, ba), (wb, bb), (wc, bc)], decisions=decisions, with_acts=True)
        out = out.reshape(B * n1, 256)
        g = None
        if grads:
            g = list(torch.autograd.grad(out, leaves, c(self.ct if ct is None else ct)))
            g[0], g[1] = g[0].reshape(B * n1, 256), g[1].reshape(B * n2, 256)
        return out.detach(), [a.detach().reshape(B * n1 * 16, 256) for a in acts], g

    def keep_mask(self, knn, par64):
        """clear_of_zero on this case's directions: (keep (B n1, 256) bool, mixed).  par64: the parameters in float64 on knn's device."""
        dev = knn.device
        wn = [(par64[5], par64[6]), (par64[7], par64[8]), (par64[9], par64[10])]
        keep, mixed = clear_of_zero(self.xyz1.to(dev).double(), self.xyz2.to(dev).double(), knn, wn)
        return keep.reshape(self.B * self.n1, 256), mixed


def band_share(acts64, skip=None):
    """The share of the three layers' activations within BAND of their layer's largest magnitude of zero, from the float64 reference.
    skip: per layer a list of channels left out (channels a test sets to exactly zero)."""
    inside = total = 0
    for l, a in enumerate(acts64):
        near = a.abs() <= BAND * a.abs().max()
        if skip is not None and skip[l]:
            cols = torch.ones(a.shape[1], dtype=torch.bool, device=a.device)
            cols[skip[l]] = False
            near = near[:, cols]
        inside, total = inside + int(near.sum()), total + near.numel()
    return inside / total


def tiles_per_workgroup(B, n1, cus=256):
    """{kernel: (tiles, workgroups)} among which a sample's (or, flattened, an XCD's) tiles are dealt, from the launchers' sizing rules
    (csrc/fused_split.hip: cv_split_fill, cv_split_forward; csrc/fused_group.hip: the cost-volume launchers):
      split backward, and split forward unless B % 8 == 0:  ceil(n1 / 8) tiles on min(256 / B, tiles) workgroups per sample;
      fp32 forward and backward:                            ceil(n1 / 4) tiles on min(512 / B, tiles) workgroups per sample;
      split forward with B % 8 == 0:                        (B / 8) ceil(n1 / 8) tiles on min(cus / 8, tiles) workgroups per XCD."""
    t8, t4 = -(-n1 // 8), -(-n1 // 4)
    res = {"split_bwd": (t8, min(max(256 // B, 1), t8)), "fp32": (t4, min(max(512 // B, 1), t4))}
    if B % 8 == 0:
        tx = (B // 8) * t8
        res["split_fwd"] = (tx, min(max(cus // 8, 1), tx))
    else:
        res["split_fwd"] = res["split_bwd"]
    return res
