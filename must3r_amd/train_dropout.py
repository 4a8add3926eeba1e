"""Memory dropout for the trainable decoder: the random token dropout of the reference's training recipe (``CausalMUSt3R(..., mem_dropout=0.1)``,
must3r/model/decoder.py:388-433, :466-494, :537-538; must3r/model/blocks/dropout.py) on the key masks of the fp32 attention kernels::

    dec = CausalMUSt3R.from_decoder(native_decoder, mem_dropout=0.1)                 # dropout_mode='temporary', protected_imgs=1, as the released recipe
    mem, pts0 = dec(x0, pos0, shape0)
    mem, pts1 = dec(x1, pos1, shape1, mem)                                          # view i of the call does not see a random subset of the rows before it
    _, pts = dec(x, pos, shape, mem, render=True)                                   # one random subset of the memory is hidden from all views
    loss(pts).backward()
    native_decoder.load_state_dict(dec.state_dict(), strict=True)

The reference hides rows with a boolean ``[B nimgs, heads, N, Nk]`` attention mask (or gathers the kept rows, in a render).  Here a draw becomes one row of
packed bits per view position of the call (``train_attention.pack_key_mask``), shared by all scenes, layers and heads, on top of the causal view table
(``must3r_hip_cross_sublayer_masked_*``, include/must3r_hip.h "ABI 21, additive"): the kernels test the bit of the key a lane already holds and skip a key tile
whose 64 bits are all zero.  A dropped row gets no gradient from the views it is hidden from -- the reference's unselected rows get zero gradient either way.

``MemoryDropoutSelector`` and ``TemporaryMemoryDropoutSelector`` are the reference's two selectors on torch tensors of any device: the same ``torch.rand`` /
``torch.randperm`` calls in the same order, so that under the same seed on the CPU they return the reference's ``sel`` / ``not_sel`` lists exactly -- including
what the reference's ``not_sel`` really holds (``MemoryDropoutSelector.draw``).

``dropout_mode='temporary'`` (the recipe's): in an update view i draws over the ``Nm + i N`` rows it can see, the first ``protected_tokens`` exempt; the
reference's loop bound ``range(len(mem_not_sel) - 1)`` is kept, so the last view of a call is not masked and a lone view never is, though its draw still
consumes the generator.  In a render one draw over the ``Nm`` rows is shared by all views: they see the rows of ``sel`` (a mask row, not the reference's gather: the same mathematics).  The whole mode runs
WITHOUT A HOST SYNCHRONISATION: the number of rows to drop stays a device scalar (ranks in the permutation and among the kept rows are compared with it on the device), and
the masks are built and packed on the device; which views name a mask row depends on shapes alone.
``dropout_mode='permanent'``: the nested draw gives view i the rows dropped by the views before it, and after the update the memory and its labels are compacted
to the rows the last draw kept (torch indexing under autograd; the rows stay in ascending order, so the causal prefixes of later calls stay valid).  The shape
of the memory then depends on the draw: this mode reads the kept rows on the host, once per view of a call.  A render applies no dropout.
Like the reference, dropout does not look at ``.training``.  ``mem_dropout == 0`` is ``train_decoder.CausalMUSt3R``, bit for bit.
"""
import torch
import torch.nn as nn

from . import train_decoder as TD
from .train_attention import pack_key_mask


class MemoryDropoutSelector(nn.Module):
    """The reference's selector of the permanent mode (blocks/dropout.py:6-64).  ``p < 1``: every unprotected row is dropped with probability p (the count is
    drawn, then a random permutation chooses the rows); ``p >= 1``: keep p rows (a host integer)."""

    def __init__(self, p=0.0, generator=None):
        super().__init__()
        self.p, self.generator = p, generator

    def draw(self, N, protected=0, device="cuda", p=None):
        """``(in_sel, in_not_sel)``, bool ``[N]`` on ``device``: membership in the reference's ``sel`` and ``not_sel`` lists, or ``None`` where nothing is drawn
        (no unprotected row).  The random calls of the reference's ``sel`` in its order.  With ``count`` rows to drop, ``sel`` is ``perm[count:]`` sorted;
        the reference then takes ``not_sel`` from the ALREADY SORTED ``sel`` (dropout.py:21-22), so the rows it reports as dropped -- the ones the temporary
        mode hides -- are the first ``count`` kept rows in ascending order, not the complement.  Restated as it is.  ``count`` stays a device scalar and
        the ranks come from a scatter and a cumulative sum: no host synchronisation."""
        p = self.p if p is None else p
        N_x = N - protected
        if N_x <= 0:
            return None
        if p < 1:
            count = torch.sum(torch.rand(N_x, device=device, generator=self.generator) < p)
        else:
            count = max(0, min(N - p, N_x))
        perm = torch.randperm(N_x, device=device, generator=self.generator)
        rank = torch.empty_like(perm)
        rank[perm] = torch.arange(N_x, device=perm.device, dtype=perm.dtype)      # rank[r]: where row r stands in the permutation
        in_sel = rank >= count
        in_not_sel = in_sel & (torch.cumsum(in_sel, dim=0) <= count)
        if protected > 0:
            head = torch.ones(protected, dtype=torch.bool, device=in_sel.device)
            in_sel, in_not_sel = torch.cat([head, in_sel]), torch.cat([~head, in_not_sel])
        return in_sel, in_not_sel

    def keep(self, N, protected=0, device="cuda", p=None):
        """bool ``[N]``: the rows a view still sees after a draw over its N rows (not in ``not_sel``), or ``None`` where nothing is drawn"""
        d = self.draw(N, protected, device, p)
        return None if d is None else ~d[1]

    def sel(self, N, protected=0, device="cuda", p=None):
        """``(sel, not_sel)`` in ascending order: the reference's lists (reads their sizes on the host)"""
        d = self.draw(N, protected, device, p)
        if d is None:
            return torch.arange(N, device=device), torch.zeros((0,), device=device, dtype=torch.int)
        return torch.nonzero(d[0]).view(-1), torch.nonzero(d[1]).view(-1)

    def forward(self, Nm, nimgs, N, protected=0, device="cuda", p=None):
        """The nested draw of an update of ``nimgs`` views of N tokens over Nm memory rows: lists of ``nimgs + 1`` index tensors into the ``Nm + nimgs N``
        key rows; ``sel[i + 1]`` are the rows that survive view i's draw, ``not_sel[i + 1]`` all rows dropped up to it."""
        p = self.p if p is None else p
        if p == 0.0:
            return None, None
        assert nimgs > 0
        sel, not_sel = [torch.arange(Nm, device=device)], [torch.arange(0, device=device)]
        for i in range(nimgs):
            sel_prev, not_sel_prev = sel[-1], not_sel[-1]
            N_prev = len(sel_prev)
            seli, not_seli = self.sel(N_prev + N, protected, device, p=p)
            keep_new, discard_new = seli >= N_prev, not_seli >= N_prev
            old_keep, old_discard = sel_prev[seli[~keep_new]], sel_prev[not_seli[~discard_new]]
            offset = (Nm + i * N) - N_prev
            sel.append(torch.cat([old_keep, seli[keep_new] + offset]))
            not_sel.append(torch.cat([not_sel_prev, old_discard, not_seli[discard_new] + offset]))
        return sel, not_sel


class TemporaryMemoryDropoutSelector(MemoryDropoutSelector):
    """The reference's selector of the temporary mode (blocks/dropout.py:67-84): view i draws afresh over the ``Nm + i N`` rows before it."""

    def forward(self, Nm, nimgs, N, protected=0, device="cuda", p=None):
        p = self.p if p is None else p
        if p == 0.0:
            return None, None
        sel, not_sel = [], []
        for i in range(nimgs):
            mem_cnt = Nm + i * N
            seli, not_seli = self.sel(mem_cnt, protected, device, p=p)
            sel.append(torch.cat([seli, torch.arange(N, device=device) + mem_cnt]))
            not_sel.append(not_seli)
        return sel, not_sel

    def keeps(self, Nm, nimgs, N, protected=0, device="cuda"):
        """``forward`` as keep masks: per view bool ``[Nm + i N]`` or ``None`` (nothing drawn); the same random calls, no host synchronisation."""
        return [self.keep(Nm + i * N, protected, device) for i in range(nimgs)]


def _keep_from_dropped(not_sel, Nk, device):
    keep = torch.ones(Nk, dtype=torch.bool, device=device)
    keep[not_sel.to(device=device, dtype=torch.int64)] = False
    return keep


class CausalMUSt3R(TD.CausalMUSt3R):
    """``train_decoder.CausalMUSt3R`` with the reference's memory dropout (decoder.py:353-553); the same parameters under the same state-dict keys.
    ``generator``: of the device the model runs on (the draws are made there, as the reference's), ``None`` for the global one."""

    def __init__(self, protected_imgs=1, mem_dropout=0.0, dropout_mode="temporary", generator=None, **kw):
        super().__init__(protected_imgs=protected_imgs, mem_dropout=0.0, **kw)
        if dropout_mode == "permanent":
            self.mem_dropout = MemoryDropoutSelector(mem_dropout, generator)
        elif dropout_mode == "temporary":
            self.mem_dropout = TemporaryMemoryDropoutSelector(mem_dropout, generator)
        else:
            raise ValueError(f"Invalid dropout mode = {dropout_mode}")
        if float(mem_dropout) < 0:
            raise ValueError(f"CausalMUSt3R: mem_dropout {mem_dropout} is negative")
        self.dropout_mode = dropout_mode

    def draw(self, Nm, nimgs, N, protected, device, render):
        """The selection of one call, overridable: ``(keeps, compact)`` -- ``keeps`` a list of bool tensors over a prefix of the call's key rows (``None``: that
        view position draws nothing), one per view of an update (permanent mode: ``nimgs + 1``, the reference's lists) or one for a render; ``compact`` the
        rows the memory keeps after a permanent update, else ``None``.  ``None`` where the call applies no dropout."""
        if render:
            if self.dropout_mode != "temporary":
                return None
            d = self.mem_dropout.draw(Nm, protected, device)      # the reference gathers the rows of sel[0] (decoder.py:478)
            return [None if d is None else d[0]], None
        if self.dropout_mode == "temporary":
            return self.mem_dropout.keeps(Nm, nimgs, N, protected, device), None
        return self._from_lists(*self.mem_dropout(Nm, nimgs, N, protected, device), Nm + nimgs * N, device, False)

    def _from_lists(self, sel, not_sel, Nk, device, render):
        """a recorded ``(sel, not_sel)`` of the reference's selector as ``(keeps, compact)``: an update hides ``not_sel[i]`` from view i, a render keeps ``sel[0]``"""
        if render:
            return [~_keep_from_dropped(sel[0], Nk, device)], None
        keeps = [_keep_from_dropped(ns, Nk, device) if ns.numel() else None for ns in not_sel]
        compact = sel[-1].to(device=device, dtype=torch.int64) if self.dropout_mode == "permanent" else None
        return keeps, compact

    def _cross_mask(self, keeps, B, V, Nk, render, device):
        """``(key_mask, view_mask)`` of a call from its keep masks: one packed row per masked view position, shared by the scenes.  An update masks the views
        ``range(len(keeps) - 1)`` (decoder.py:404), a render all views with its one draw."""
        rows, index = [], {}
        for i in ([0] if render else range(len(keeps) - 1)):
            if i < len(keeps) and keeps[i] is not None:
                k = keeps[i]
                index[i] = len(rows)
                rows.append(k if k.numel() == Nk else torch.cat([k, torch.ones(Nk - k.numel(), dtype=torch.bool, device=device)]))
        if not rows:
            return None, None
        view_mask = [index.get(0 if render else j, -1) for _ in range(B) for j in range(V)]
        return pack_key_mask(torch.stack(rows)), view_mask

    def forward(self, x, pos, true_shape, current_mem=None, render=False, return_tokens=False, selection=None, img_shape=None):
        """``train_decoder.MUSt3R.forward`` with dropout.  ``selection``: the ``(sel, not_sel)`` lists the reference's selector returned for this call (index
        tensors on any device) instead of a draw of this module's -- a recorded draw can be replayed.  In the permanent mode the memory and the labels of
        the returned tuple hold the kept rows only.  ``img_shape``: ``train_decoder.MUSt3R.forward``'s."""
        p = self.mem_dropout.p
        if not p > 0.0:
            return super().forward(x, pos, true_shape, current_mem, render, return_tokens, img_shape=img_shape)
        if render and self.dropout_mode != "temporary":
            return super().forward(x, pos, true_shape, current_mem, render, return_tokens, img_shape=img_shape)
        TD._dev(x, "x")
        if x.ndim != 4:
            raise ValueError(f"MUSt3R: x of shape {tuple(x.shape)}, expected [B, nimgs, N, {self.enc_embed_dim}]")
        if render and current_mem is None:
            raise ValueError("MUSt3R: a render needs a memory")
        B, V, N, _ = (int(s) for s in x.shape)
        if current_mem is None:
            Nm, prot_imgs, prot_tokens = 0, 0, 0
        else:
            Nm, prot_imgs, prot_tokens = int(current_mem[0][0].shape[1]), int(current_mem[3]), int(current_mem[4])
        if not render:   # the protected tokens of THIS call's tuple (decoder.py:456-459)
            _, prot_tokens = self._memory_tail(0, 0, prot_imgs, prot_tokens, V, N)
        Nk = Nm if render else Nm + V * N
        if selection is not None:
            keeps, compact = self._from_lists(selection[0], selection[1], Nk, x.device, render)
        else:
            keeps, compact = self.draw(Nm, V, N, prot_tokens, x.device, render)
        masked = render or Nm > 0 or V > 1          # a lone first view attends its own tokens, unmasked (decoder.py:498)
        key_mask, view_mask = self._cross_mask(keeps, B, V, Nk, render, x.device) if masked else (None, None)
        out = super().forward(x, pos, true_shape, current_mem, render, return_tokens, key_mask, view_mask, img_shape)
        if compact is None or render:
            return out
        mem, labels, *tail = out[0]
        mem = ([m[:, compact] for m in mem], labels[:, compact], *tail)
        return (mem, *out[1:])
