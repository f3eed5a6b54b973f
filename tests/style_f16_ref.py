"""CPU emulation of the mixed-precision multi-style loss (csrc/style_f16.hip, mstg_hip/style_f16.py) in float64 arithmetic with the
device's roundings at the device's points, and the shared inputs of its tests.

Forward: the image and the weights rounded to fp16, every ReLU output rounded to fp16 (max-pool picks among rounded values, Gram
matrices and the loss stay unrounded: the device keeps them in fp32).  Backward: the weights rounded fp32 -> bf16, every gradient
that the device stores between two kernels rounded to bf16 at the same point: behind each Gram backward (incoming gradient added,
ReLU mask applied), behind each convolution input gradient (ReLU mask of the layer's input applied), behind each pool backward
(exact: it routes rounded values).  dL/dy is left unrounded (fp32 on the device).

``round_fp16`` / ``round_bf16`` are written from the formats' definitions (round to nearest even at 11 / 8 significant bits, fp16
subnormals below 2^-14, overflow to infinity), not with torch's casts: tests/test_style_f16_cpu.py checks them against the casts.
"""
import torch
import torch.nn.functional as F

from oracle import restatement as R


def _round_to(t, sig_bits, min_exp, max_finite):
    t = t.double()
    m, e = torch.frexp(t)  # t = m * 2^e, 0.5 <= |m| < 1: the leading bit has weight 2^(e - 1)
    ulp_exp = torch.clamp(e - 1, min=min_exp) - (sig_bits - 1)
    ulp = torch.ldexp(torch.ones_like(t), ulp_exp)
    r = torch.round(t / ulp) * ulp  # torch.round: half to even; t / ulp is exact (a power of two)
    # the largest finite value plus half an ulp and beyond rounds to infinity
    half_ulp_top = 2.0 ** (torch.frexp(torch.tensor(max_finite, dtype=torch.float64))[1].item() - 1 - (sig_bits - 1)) / 2
    r = torch.where(t.abs() >= max_finite + half_ulp_top, torch.sign(t) * float("inf"), r)
    return torch.where(torch.isfinite(t), r, t)


def round_fp16(t):
    return _round_to(t, 11, -14, 65504.0)


def round_bf16(t):
    return _round_to(t, 8, -126, 3.3895313892515355e38)


# ---- shared inputs of the whole-loss tests ---------------------------------------------------------------------------------------
SHAPE, WIDTH_DIV = (2, 3, 32, 32), 4
WEIGHTS3 = (0.5, 0.3, 0.2)


def loss_inputs():
    """(state dict, y, three style references with clearly different statistics) of the whole-loss tests."""
    sd = R.make_state_dict(R.vgg_spec(WIDTH_DIV), 77)
    y = R.make_input(SHAPE, 79)
    styles = [(R.make_input(SHAPE, 80 + k) * (0.25 + 0.2 * k) + (0.5 - 0.4 * k)).clamp(-1, 1) for k in range(3)]
    return sd, y, styles


def conv_indices():
    """plan of the stack: "M" or the convolution's index, as style_loss.VGGFeatures.plan"""
    plan, i = [], 0
    for c in R.VGG_CFG:
        if c == "M":
            plan.append("M")
        else:
            plan.append(i)
            i += 1
    return plan


def emulate(sd, y, styles, weights, with_grad=True):
    """dict(loss, feats [4 x (N,C,H,W) float64], dy) of the emulated mixed path; ``sd``: the fp32 weights."""
    plan = conv_indices()
    w16 = {k: round_fp16(v) for k, v in sd.items() if k.endswith("weight")}
    wb = {k: round_bf16(v) for k, v in sd.items() if k.endswith("weight")}
    bias = {k: v.double() for k, v in sd.items() if k.endswith("bias")}  # fp32 on the device

    def forward(x):
        h, acts, pools = round_fp16(x), [], []
        for item in plan:
            if item == "M":
                h, idx = F.max_pool2d(h, 2, return_indices=True)
                pools.append((h, idx))
                continue
            h = round_fp16(F.relu(F.conv2d(h, w16[f"conv{item}.weight"], bias[f"conv{item}.bias"], padding=1)))
            acts.append(h)
        return acts, pools

    def targets_of():
        per = [[R.gram_matrix(a[i]).mean(dim=0, keepdim=True) for i in R.VGG_TAPS] for a, _ in (forward(s) for s in styles)]
        return [sum(w * gs[l] for w, gs in zip(weights, per)) for l in range(len(R.VGG_TAPS))]

    acts, pools = forward(y)
    targets = targets_of()
    grams = [R.gram_matrix(acts[i]) for i in R.VGG_TAPS]
    loss = sum(((g - t) ** 2).mean() for g, t in zip(grams, targets))
    out = {"loss": loss, "feats": [acts[i] for i in R.VGG_TAPS], "dy": None}
    if not with_grad:
        return out
    tap_of = {ci: t for t, ci in enumerate(R.VGG_TAPS)}
    g, npool = None, len(pools)
    for pos in range(len(plan) - 1, -1, -1):
        item = plan[pos]
        if item == "M":
            npool -= 1
            before = plan[pos - 1]
            g = F.max_unpool2d(g, pools[npool][1], 2, output_size=acts[before].shape[-2:])
            if before not in tap_of:
                g = g * (acts[before] > 0)
            g = round_bf16(g)
            continue
        if item in tap_of:
            f = acts[item]
            n, c, hh, ww = f.shape
            gm, t = grams[tap_of[item]], targets[tap_of[item]]
            dg = 2.0 * (gm - t) / gm.numel()
            s = dg + dg.transpose(1, 2)
            df = torch.bmm(s, f.reshape(n, c, hh * ww)).reshape(n, c, hh, ww) / (c * hh * ww)
            if g is not None:
                df = df + g
            g = round_bf16(df * (f > 0))
        w = wb[f"conv{item}.weight"]
        g = F.conv_transpose2d(g, w, None, padding=1)
        if item == 0:
            out["dy"] = g
            return out
        src = plan[pos - 1]
        if src != "M":
            g = g * (acts[src] > 0)
        g = round_bf16(g)
    raise AssertionError("empty plan")


def yardstick(sd, y, styles, weights):
    """float64 loss, tap features and dL/dy of oracle/restatement.py on the fp16-rounded weights ``sd`` (what the device holds)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    yd = y.double().requires_grad_(True)
    loss = R.multi_style_gram_loss(sd64, yd, [s.double() for s in styles], list(weights))
    loss.backward()
    with torch.no_grad():
        feats = R.vgg_features(sd64, y.double())
    return {"loss": loss.detach(), "feats": feats, "dy": yd.grad}


def rounded_weights(sd):
    """fp16-rounded weights, fp32 biases (the device keeps the bias in fp32)"""
    return {k: (v.half().float() if k.endswith("weight") else v.clone()) for k, v in sd.items()}
