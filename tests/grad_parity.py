"""The parity bound of the training tests (test_head_grad_gpu.py, test_attn_grad_gpu.py, test_block_grad_gpu.py, test_cross_grad_gpu.py) and the table they
keep under profiles/: a GPU result is held to ``e_gpu <= 4 e_ref + 32 * 2^-24 * m`` against the fp64 yardstick, where ``e_ref`` is the error of the same
formulas under fp32 CPU autograd and ``m`` the magnitude of the fp64 tensor.  ``compare_rounded`` is the same form for a kernel whose roundings are fixed by
contract (tests/test_attn16_gpu.py): against the fp64 run of the rounded arithmetic itself, on a quantile of (row, head) segments."""
import torch

U = 2.0 ** -24


def compare(rows, tag, got, g64, g32, mags=None):
    """Every tensor of ``g64`` (fp64 truth) against ``got`` (the GPU's) and ``g32`` (fp32 CPU autograd): dtype and shape, both finite, then the bound.
    ``mags``: name -> m where max|g64| is not the scale of the tensor.  A row per tensor is printed and appended to ``rows`` before anything is asserted on
    the errors: (tag, name, m, e_gpu and e_ref in units of 2^-24 m, e_gpu / bound)."""
    bad = []
    for k in g64:
        g = got[k].detach().cpu()
        assert g.dtype == torch.float32 and g.shape == g64[k].shape, (tag, k, g.dtype, g.shape)
        assert bool(torch.isfinite(g64[k]).all()) and bool(torch.isfinite(g).all()), (tag, k, "not finite")
        m = float(g64[k].abs().max()) if not (mags and k in mags) else mags[k]
        e_gpu = float((g.double() - g64[k]).abs().max())
        e_ref = float((g32[k].double() - g64[k]).abs().max())
        bound = 4 * e_ref + 32 * U * m
        unit = U * m if m > 0 else 1.0
        ratio = e_gpu / bound if bound > 0 else (0.0 if e_gpu == 0 else float("inf"))
        rows.append((tag, k, m, e_gpu / unit, e_ref / unit, ratio))
        print(f"{tag} {k}: m {m:.4e} e_gpu {e_gpu / unit:.2f} e_ref {e_ref / unit:.2f} (units of 2^-24 m) e_gpu / bound {ratio:.3f}")
        if not e_gpu <= bound:
            bad.append((k, e_gpu, e_ref, bound))
    assert not bad, (tag, bad)


def segment_errors(t, y64, heads, counted=None):
    """max |t - y64| of every (row, head) segment of a [R, heads * W] tensor, flat, over the rows ``counted`` (bool [R]) names, or all rows"""
    e = (t.double() - y64).abs().reshape(y64.shape[0], heads, -1).max(-1).values
    return (e if counted is None else e[counted]).reshape(-1)


def compare_rounded(rows, tag, got, y64, r32, heads, quantile=0.9, counted=None):
    """The rule for kernels with rounding points fixed by contract.  ``y64`` is the fp64 run of the SAME rounded arithmetic, so what is left in
    ``got - y64`` is the fp32 accumulation error -- except where a value lies so near a rounding boundary that its fp32 and fp64 forms round to different
    neighbours, which costs a whole ulp of the narrow format in that place and is legitimate.  Such places are rare and live in one head, so the unit is the
    (row, head) segment of a tensor [R, heads * W], a segment's error is its max |. - y64|, and the rule holds a QUANTILE of the segment errors:
    ``q(e_gpu) <= 4 q(e_ref) + 32 * 2^-24 * m`` with ``e_ref`` the segment errors of ``r32`` (the fp32 CPU run of the same arithmetic) and m = max|y64|.
    The share ``1 - quantile`` that it steps over is a condition of the rule, not something measured: it is not to be raised for a run that fails.
    ``counted``: name -> bool [R], the rows whose segments count (all, where a name is missing): the rows the operation writes; the others are exact zeros
    that the callers hold to that elsewhere, and would only dilute the quantile.  A row per tensor is printed and appended to ``rows`` before anything is
    asserted on the errors: (tag, name, m, q(e_gpu) and q(e_ref) in units of 2^-24 m, q(e_gpu) / bound, the share of ``got``'s segments above the bound)."""
    bad = []
    for k in y64:
        g = got[k].detach().cpu()
        assert g.dtype == torch.float32 and g.shape == y64[k].shape, (tag, k, g.dtype, g.shape)
        assert bool(torch.isfinite(y64[k]).all()) and bool(torch.isfinite(g).all()), (tag, k, "not finite")
        c = None if counted is None else counted.get(k)
        eg, er = segment_errors(g, y64[k], heads, c), segment_errors(r32[k], y64[k], heads, c)
        assert eg.numel() > 0, (tag, k, "no segment counted")
        m = float(y64[k].abs().max())
        q_gpu, q_ref = float(torch.quantile(eg, quantile)), float(torch.quantile(er, quantile))
        bound = 4 * q_ref + 32 * U * m
        unit = U * m if m > 0 else 1.0
        ratio = q_gpu / bound if bound > 0 else (0.0 if q_gpu == 0 else float("inf"))
        share = float((eg > bound).double().mean())
        rows.append((tag, k, m, q_gpu / unit, q_ref / unit, ratio, share))
        print(f"{tag} {k}: m {m:.4e} q{quantile:g} e_gpu {q_gpu / unit:.2f} e_ref {q_ref / unit:.2f} (units of 2^-24 m, {eg.numel()} segments) "
              f"q e_gpu / bound {ratio:.3f} share above the bound {share:.4f}")
        if not q_gpu <= bound:
            bad.append((k, q_gpu, q_ref, bound, share))
    assert not bad, (tag, bad)


def append_rounded_table(path, header_lines, rows, widths, mode="a"):
    """``rows`` of ``compare_rounded`` appended to the table at ``path`` (nothing without a path or rows; ``mode`` "w" starts the file) as a section of its
    own: the comment lines of ``header_lines``, the column titles, a line per row, the worst ratio and the worst share."""
    if not (rows and path):
        return
    wc, wt = widths
    with open(path, mode) as f:
        f.writelines(line + "\n" for line in header_lines)
        f.write(f"{'case':<{wc}}{'tensor':<{wt}}{'m':>12}{'q e_gpu':>10}{'q e_ref':>10}{'ratio':>8}{'share':>8}\n")
        for r in rows:
            f.write(f"{r[0]:<{wc}}{r[1]:<{wt}}{r[2]:>12.4e}{r[3]:>10.2f}{r[4]:>10.2f}{r[5]:>8.3f}{r[6]:>8.4f}\n")
        f.write(f"# worst ratio {max(r[5] for r in rows):.3f}, worst share above the bound {max(r[6] for r in rows):.4f}\n")


def write_table(path, header_lines, rows, widths, magnitude="max|g64|", worst=True):
    """``rows`` of ``compare`` as a table at ``path`` (nothing without a path or rows): the comment lines of ``header_lines``, the column titles, a line per
    row, and with ``worst`` the worst ratio.  ``widths``: of the case and the tensor column; ``magnitude``: the title of the third."""
    if not (rows and path):
        return
    wc, wt = widths
    with open(path, "w") as f:
        f.writelines(line + "\n" for line in header_lines)
        f.write(f"{'case':<{wc}}{'tensor':<{wt}}{magnitude:>12}{'e_gpu':>10}{'e_ref':>10}{'ratio':>8}\n")
        for r in rows:
            f.write(f"{r[0]:<{wc}}{r[1]:<{wt}}{r[2]:>12.4e}{r[3]:>10.2f}{r[4]:>10.2f}{r[5]:>8.3f}\n")
        if worst:
            f.write(f"# worst ratio {max(r[5] for r in rows):.3f}\n")
