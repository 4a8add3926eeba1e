"""The parity bound of the training tests (test_head_grad_gpu.py, test_attn_grad_gpu.py, test_block_grad_gpu.py, test_cross_grad_gpu.py) and the table they
keep under profiles/: a GPU result is held to ``e_gpu <= 4 e_ref + 32 * 2^-24 * m`` against the fp64 yardstick, where ``e_ref`` is the error of the same
formulas under fp32 CPU autograd and ``m`` the magnitude of the fp64 tensor."""
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
