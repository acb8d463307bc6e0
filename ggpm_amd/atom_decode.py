"""The atom level of the teacher-forced decoder as ONE autograd node.

Inside ``HierMPNDecoder.forward`` the reference calls ``IncHierMPNEncoder.forward`` once per decode step
(ggpm/decoder.py:201-222); its first block (ggpm/encoder.py:235-239) recomputes, on the atom level, the bond messages
among the atoms the previous step revealed (``diterG`` interacting iterations of ``sparse_forward``) and the vectors of
those atoms (``IncMPNEncoder.forward``, ggpm/encoder.py:165-179).  This level is the part of the decoder that is truly
sequential in the step index (the two tree-side levels are not, see ``DecodeSchedule._level_plan``).

Teacher forcing fixes every index of that loop in advance, so ``AtomPlan`` builds all of them on the host, once per
batch: per step the frozen mask, the masked predecessor CSR of the step's bonds and its transpose, the masked
incoming-message CSR of the step's atoms and its transpose, and -- composed with the scatter into the zeroed node
buffer the reference rebuilds at every step -- where each pooled cluster vector (``embed_sub_tree``) and each
attachment candidate (``enum_attach``) reads the step's atom vectors.  ``atom_decode`` then runs the whole loop as one
``torch.autograd.Function`` whose forward and backward call the C ABI directly (``ggpm_decode_steps_*``,
``ggpm_segment_sum``, ``ggpm_gemm*``): no per-step autograd graph, no per-step index kernels, the gate input
projections of ALL bonds computed once (they are depth- and step-invariant one-hot look-ups), and every weight gradient
formed once per call (the read-out's from the stacked rows of all steps, the input halves from the summed ``dX``).

Compact steps: a step recomputes a few hundred of the level's thousands of bond messages, so its ``sparse_forward`` runs
on the step's COMPACT row set -- the step's bonds plus the frozen older bonds they read, renumbered 0..n-1 with
host-built local CSRs -- and not on every row of the level under a frozen mask: a step's frozen rows are gathered from
the blocks of the earlier steps that produced them, their gradients scatter-added back there (``ggpm_gather_rows`` /
``ggpm_scatter_rows``, ``AtomPlan.compact_tables``), the depth kernels launch ~1/8 of the row tiles and the hidden-half
weight-gradient contractions shrink by the same factor.  Same arithmetic per row as a level-wide step.  The step loops
themselves are csrc/decode.hip's; tests/test_decode_steps_gpu.py checks them against fp64 and, bit for bit, against the
same steps issued one public call at a time.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import List

import numpy as np
import torch

from . import _dev, _lib, fused
from . import functional as F_


def _csr_from_lists(counts: np.ndarray, flat: np.ndarray):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), flat.astype(np.int32)


def _transpose(rows: np.ndarray, cols: np.ndarray, ncols: int):
    """(row, col) entry lists -> CSR of the transpose (rows of the result = columns), entries ascending."""
    order = np.lexsort((rows, cols))
    return (np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=ncols))]).astype(np.int32),
            rows[order].astype(np.int32))


class AtomPlan:
    """Host-built index tables of the atom-level decode loop (see the module docstring)."""

    def __init__(self, schedule, n_gnodes: int, n_gmess: int, full: bool = False):
        """``full``: also build the level-wide per-step tables (frozen mask and CSRs over all E1 rows of every step).  They are
        the reference of tests/test_oracle_golden.py::test_atom_plan_compact_row_sets_match_the_level_wide_tables; nothing on
        the device reads them (the level-wide mask ``frozen`` is not uploaded), and they are the larger half of the build."""
        P, steps = schedule.plan, schedule.steps
        self._native, self._schedule, self._raw_cache = None, None, None
        self.T, self.N1, self.E1 = len(steps), n_gnodes, n_gmess
        self.full = full = bool(full)
        self.ok = all(len(st["atoms"]) > 0 for st in steps)          # (the reference keeps a stale node buffer otherwise)
        ints: List[np.ndarray] = []
        self.where = {}
        fill = [0]

        def put(key, a):
            a = np.asarray(a, dtype=np.int32).reshape(-1)
            self.where[key] = (fill[0], len(a))
            fill[0] += len(a)
            ints.append(a)

        frozen = np.ones((self.T if full else 0, n_gmess), dtype=np.uint8)
        frozen_loc: List[np.ndarray] = []                     # compact steps: mask over the step's local rows
        self.nloc, self.floc_off = [], [0]
        self._raw, self._ct = [], {}                          # per step (rows, mask, incoming-message table, pool table)
        aoff, boff, ioff = P["atom_off"], P["bond_off"], P["inst_off"]
        self.aoff, self.ioff = aoff, ioff
        # candidate atoms of all steps, grouped by atoms-per-candidate k first, then by step: one contiguous block per k
        groups = sorted({len(icls) for st in steps for (_, icls, _, _) in st["assm"]})
        cand_pos = {k: [] for k in groups}
        cand_meta = {k: dict(icls=[], nth=[], dest=[]) for k in groups}
        per_step_cands = []
        pred_i = 0
        for t, st in enumerate(steps):
            bonds = np.asarray(st["bonds"], dtype=np.int64)
            atoms = np.asarray(st["atoms"], dtype=np.int64)
            # predecessor CSR over all E1 rows (only this step's bonds have entries) and its transpose
            order = np.argsort(bonds, kind="stable")
            tab = P["g_bgraph"][boff[t]:boff[t + 1]][order]
            cnt = (tab > 0).sum(axis=1)
            if full:
                frozen[t, bonds] = 0
                counts = np.zeros(n_gmess, dtype=np.int64)
                counts[bonds[order]] = cnt
                rp, col = _csr_from_lists(counts, tab[tab > 0])
                put(("pred_rp", t), rp); put(("pred_col", t), col)
                rpT, colT = _transpose(np.repeat(bonds[order], cnt), tab[tab > 0], n_gmess)
                put(("succ_rp", t), rpT); put(("succ_col", t), colT)
            # the same two CSRs over the step's compact row set: its bonds + the frozen rows they read + the null row
            rows = np.union1d(np.union1d(bonds, tab[tab > 0]), [0]).astype(np.int64)
            n = len(rows)
            lpos = np.full(n_gmess, -1, dtype=np.int64)
            lpos[rows] = np.arange(n)
            lcounts = np.zeros(n, dtype=np.int64)
            lcounts[lpos[bonds[order]]] = cnt                  # (ascending global id = ascending local id)
            rp, col = _csr_from_lists(lcounts, lpos[tab[tab > 0]])
            put(("lpred_rp", t), rp); put(("lpred_col", t), col)
            rpT, colT = _transpose(np.repeat(lpos[bonds[order]], cnt), lpos[tab[tab > 0]], n)
            put(("lsucc_rp", t), rpT); put(("lsucc_col", t), colT)
            fl = np.ones(n, dtype=np.uint8)
            fl[lpos[bonds]] = 0
            frozen_loc.append(fl)
            self.nloc.append(n)
            self.floc_off.append(self.floc_off[-1] + (n + 15) // 16 * 16)
            put(("rows", t), rows)                             # local -> level row
            # incoming messages of the step's atoms (rows local to the step) and the transpose (rows = messages)
            atab = P["g_agraph"][aoff[t]:aoff[t + 1]]
            if full:
                acnt = (atab > 0).sum(axis=1)
                rp, col = _csr_from_lists(acnt, atab[atab > 0])
                put(("agr_rp", t), rp); put(("agr_col", t), col)
                rpT, colT = _transpose(np.repeat(np.arange(len(atoms)), acnt), atab[atab > 0], n_gmess)
                put(("agrT_rp", t), rpT); put(("agrT_col", t), colT)
            # pooled cluster vectors of the step's visits read the step's atom vectors (other atoms' rows are zero in
            # the node buffer the reference rebuilds every step)
            pos = np.full(n_gnodes, -1, dtype=np.int64)
            pos[atoms] = np.arange(len(atoms))
            ptab = P["pool"][ioff[t]:ioff[t + 1]]
            loc = np.where(ptab > 0, pos[ptab], -1)
            if full:
                pcnt = (loc >= 0).sum(axis=1)
                rp, col = _csr_from_lists(pcnt, loc[loc >= 0])
                put(("pool_rp", t), rp); put(("pool_col", t), col)
                rpT, colT = _transpose(np.repeat(np.arange(len(ptab)), pcnt), loc[loc >= 0], len(atoms))
                put(("poolT_rp", t), rpT); put(("poolT_col", t), colT)
            self._raw.append((rows, fl, atab, loc))
            here = []
            for (cands, icls, nth, _) in st["assm"]:
                k, n = len(icls), len(cands)
                start = len(cand_pos[k])
                cand_pos[k].extend(pos[cands.reshape(-1)].tolist())
                m = cand_meta[k]
                m["icls"].extend(list(icls) * n)
                m["nth"].extend([nth] * (n * k))
                m["dest"].extend(range(pred_i * schedule.max_cls_size, pred_i * schedule.max_cls_size + n))
                here.append((k, start, n * k))
                pred_i += 1
            per_step_cands.append(here)
        # flat candidate layout: block of k = 1 rows, then k = 2 ...
        base, self.cand_blocks = 0, []
        for k in groups:
            self.cand_blocks.append((k, base, len(cand_pos[k])))
            base += len(cand_pos[k])
        self.n_cand = base
        kbase = {k: b for k, b, _ in self.cand_blocks}
        self._cand_pos, self._per_step_cands, self._kbase = cand_pos, per_step_cands, kbase
        self.step_cands = []                                  # per step: [(flat row offset, count)] + transposed scatter
        for t, here in enumerate(per_step_cands):
            segs = [(kbase[k] + start, n) for (k, start, n) in here]
            self.step_cands.append(segs)
            ns = aoff[t + 1] - aoff[t]
            for j, (k, start, n) in enumerate(here if full else ()):
                p = np.asarray(cand_pos[k][start:start + n], dtype=np.int64)
                put(("cand_pos", t, j), p)
                ok = p >= 0
                rpT, colT = _transpose(np.arange(n)[ok], p[ok], ns)
                put(("candT_rp", t, j), rpT); put(("candT_col", t, j), colT)
        self.cand_meta = {k: {n: np.asarray(v, dtype=np.int64) for n, v in m.items()} for k, m in cand_meta.items()}
        self.ints = np.concatenate(ints) if ints else np.zeros(0, np.int32)
        self.frozen = frozen
        # stacked per-step blocks: depth * n rows (stashes) / (depth + 1) * n rows (states), see row_offsets()
        self.frozen_loc = np.ones(self.floc_off[-1], dtype=np.uint8)
        for t, fl in enumerate(frozen_loc):
            self.frozen_loc[self.floc_off[t]:self.floc_off[t] + len(fl)] = fl
        self._dev = {}

    def __getstate__(self):
        """Host tables only: device copies and the descriptors that name them stay with the process that made them."""
        st = dict(self.__dict__)
        st["_dev"] = {}
        st["_schedule"] = self._schedule() if self._schedule is not None else None       # (the weak reference back: __setstate__)
        st["_ct"] = {k: dict(v, dev={}) for k, v in self._ct.items()}
        if self._native is not None:
            from .decoder import _FrozenTables
            st["_native"] = self._native if isinstance(self._native, _FrozenTables) else _FrozenTables(self._native)
            st["ints"], st["frozen_loc"] = np.array(self.ints), np.array(self.frozen_loc)
            st["cand_meta"] = {k: {n: np.array(v) for n, v in m.items()} for k, m in self.cand_meta.items()}
            st["_raw_cache"] = None
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        if self._schedule is not None:
            self._schedule = weakref.ref(self._schedule)

    # ------------------------------------------------------------------ tables built by csrc/schedule.hip
    @classmethod
    def from_native(cls, schedule, nt, n_gnodes: int, n_gmess: int) -> "AtomPlan":
        """The same object over the tables of ``ggpm_schedule_build``: ``ints`` IS the int32 device pack (so the
        addresses handed to the C drivers are offsets into one upload shared with the schedule), the compact tables for the
        (depth, gates) the build was given are already there."""
        self = cls.__new__(cls)
        sc, g = nt.scalars(), nt.get
        # (weak: the schedule owns this plan -- a strong reference back would make the pair, and with it every device table of
        # the batch, a reference cycle that only Python's collector frees)
        self._native, self._schedule = nt, weakref.ref(schedule)
        self.T, self.N1, self.E1, self.full, self.ok = sc["T"], n_gnodes, n_gmess, False, bool(sc["ok"])
        self.nloc, self.floc_off = g("nloc").tolist(), g("floc_off").tolist()
        self.aoff, self.ioff = schedule.plan["atom_off"], schedule.plan["inst_off"]
        self.ints, self.frozen_loc = nt.packs[2], g("frozen_loc")
        self.frozen = np.ones((0, n_gmess), dtype=np.uint8)
        d = nt.dir
        e32 = lambda name: d[name][1] // 4                      # element offset inside the int32 pack
        rp_off, col_off, rows_off = g("lpred_rp_off").tolist(), g("lpred_col_off").tolist(), g("rows_off").tolist()
        self.where = {}
        for t in range(self.T):
            for name, off in (("lpred_rp", rp_off), ("lsucc_rp", rp_off), ("lpred_col", col_off), ("lsucc_col", col_off),
                              ("rows", rows_off)):
                self.where[(name, t)] = (e32(name) + off[t], off[t + 1] - off[t])
        cb = g("cand_blocks").reshape(-1, 3).tolist()
        self.cand_blocks = [tuple(x) for x in cb]
        self.n_cand = sc["n_cand"]
        self.cand_meta = {k: dict(icls=g("meta_icls/%d" % k), nth=g("meta_nth/%d" % k), dest=g("meta_dest/%d" % k))
                          for k, _, _ in self.cand_blocks}
        self._kbase = {k: b for k, b, _ in self.cand_blocks}
        self._cand_pos = {k: g("cand_pos/%d" % k) for k, _, _ in self.cand_blocks}
        psc = g("step_cands").reshape(-1, 4).tolist()
        self._per_step_cands = [[] for _ in range(self.T)]
        for t, k, start, n in psc:
            self._per_step_cands[t].append((k, start, n))
        self.step_cands = [[(self._kbase[k] + start, n) for (k, start, n) in here] for here in self._per_step_cands]
        self._raw_cache, self._ct, self._dev = None, {}, {}
        if sc["depth"] > 0 and sc["gates"] > 0:
            names = ["srcF", "srcH", "agr_rp", "agr_col", "agrT_rp", "agrT_col", "pool_rp", "pool_col", "poolT_rp", "poolT_col",
                     "cand_idx", "candT_rp", "candT_col", "xrows", "xT_rp", "xT_col"]
            foff = g("foff").tolist()
            where = {}
            for name in names:
                if name in ("srcF", "srcH"):
                    for t in range(self.T):
                        where[(name, t)] = (e32(name) + foff[t], foff[t + 1] - foff[t])
                else:
                    where[name] = (e32(name), d[name][2])
            self._ct[(sc["depth"], sc["gates"])] = dict(ints=nt.packs[2], where=where, foff=foff, Ftot=sc["Ftot"], dev={},
                                                        native=True)
        return self

    def _owner(self):
        sch = self._schedule() if self._schedule is not None else None
        if sch is None:
            raise RuntimeError("AtomPlan: the DecodeSchedule these tables belong to is gone")
        return sch

    @property
    def _raw(self):
        """per step (rows, local frozen mask, incoming-message table, pool table) -- what compact_tables reads"""
        if self._raw_cache is None:
            nt, P = self._native, self._owner().plan
            rows_all, rows_off = nt.get("rows").astype(np.int64), nt.get("rows_off").tolist()
            loc = nt.get("loc").reshape(-1, P["pool"].shape[1])
            self._raw_cache = []
            for t in range(self.T):
                rows = rows_all[rows_off[t]:rows_off[t + 1]]
                fl = np.array(self.frozen_loc[self.floc_off[t]:self.floc_off[t] + len(rows)])
                self._raw_cache.append((rows, fl, P["g_agraph"][self.aoff[t]:self.aoff[t + 1]], loc[self.ioff[t]:self.ioff[t + 1]]))
        return self._raw_cache

    @_raw.setter
    def _raw(self, value):
        self._raw_cache = value

    def row_offsets(self, depth: int):
        """-> (offsets of the steps' [depth, n] blocks, offsets of their [depth + 1, n] blocks), each of length T + 1."""
        n = np.asarray(self.nloc, dtype=np.int64)
        return (np.concatenate([[0], np.cumsum(depth * n)]).tolist(),
                np.concatenate([[0], np.cumsum((depth + 1) * n)]).tolist())

    def compact_tables(self, depth: int, gates: int):
        """Host tables of the compact form that depend on the iteration count / the number of gates (cached).

        Every step leaves the final states of its n rows in slot ``depth`` of its block of the stacked state buffer.  ``F
        id`` = foff[t] + i numbers those rows over all steps; ``H id`` is the row of the same state in the stacked
        [(depth + 1) * n_t]-row blocks.  A message's state at time t is the final state of the last step <= t that
        recomputed it (zero if none did): that look-up is resolved here, once, so the device never needs a level-wide
        state -- a step's frozen rows are gathered straight from the earlier steps' blocks (``srcH``) and the read-out of
        ALL steps (incoming messages -> atoms -> pooled clusters / attachment candidates) is one CSR over the stacked
        blocks (``agr``), i.e. a handful of launches behind the loop instead of a handful per step."""
        key = (depth, gates)
        if key in self._ct:
            return self._ct[key]
        T, E1 = self.T, self.E1
        n = np.asarray(self.nloc, dtype=np.int64)
        foff = np.concatenate([[0], np.cumsum(n)])
        Ftot = int(foff[-1])
        stepof = np.repeat(np.arange(T), n)
        Hid = (depth + 1) * foff[stepof] + depth * n[stepof] + (np.arange(Ftot) - foff[stepof])
        last = np.full(E1, -1, dtype=np.int64)
        tabs, where, fill = [], {}, [0]

        def put(key_, a):
            a = np.asarray(a, dtype=np.int32).reshape(-1)
            where[key_] = (fill[0], len(a))
            fill[0] += len(a)
            tabs.append(a)

        agr_r, agr_c, pool_r, pool_c = [], [], [], []
        for t, (rows, fl, atab, loc) in enumerate(self._raw):
            sf = np.where(fl == 1, last[rows], -1)
            put(("srcF", t), sf)
            put(("srcH", t), np.where(sf >= 0, Hid[np.maximum(sf, 0)], -1))
            live = np.nonzero(fl == 0)[0]
            last[rows[live]] = foff[t] + live
            r, c = np.nonzero(atab > 0)
            f = last[atab[r, c]]
            agr_r.append(self.aoff[t] + r[f >= 0]); agr_c.append(f[f >= 0])
            r, c = np.nonzero(loc >= 0)
            pool_r.append(self.ioff[t] + r); pool_c.append(self.aoff[t] + loc[r, c])
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
        agr_r, agr_c, pool_r, pool_c = cat(agr_r), cat(agr_c), cat(pool_r), cat(pool_c)
        ns_tot, n_inst = int(self.aoff[-1]), int(self.ioff[-1])
        rp = lambda r_, nrows: np.concatenate([[0], np.cumsum(np.bincount(r_, minlength=nrows))])
        put("agr_rp", rp(agr_r, ns_tot)); put("agr_col", Hid[agr_c])                 # rows ascend already (step order)
        a, b = _transpose(agr_r, agr_c, Ftot); put("agrT_rp", a); put("agrT_col", b)
        put("pool_rp", rp(pool_r, n_inst)); put("pool_col", pool_c)
        a, b = _transpose(pool_r, pool_c, ns_tot); put("poolT_rp", a); put("poolT_col", b)
        cidx = np.full(max(self.n_cand, 1), -1, dtype=np.int64)
        for t, here in enumerate(self._per_step_cands):
            for (k, start, cnt) in here:
                pos = np.asarray(self._cand_pos[k][start:start + cnt], dtype=np.int64)
                cidx[self._kbase[k] + start:self._kbase[k] + start + cnt] = np.where(pos >= 0, self.aoff[t] + pos, -1)
        put("cand_idx", cidx)
        ok = np.nonzero(cidx >= 0)[0]
        a, b = _transpose(ok, cidx[ok], ns_tot); put("candT_rp", a); put("candT_col", b)
        xrows = np.concatenate([self.gate_rows(t, gates) for t in range(T)]).astype(np.int64)
        put("xrows", xrows)
        a, b = _transpose(np.arange(len(xrows)), xrows, gates * E1); put("xT_rp", a); put("xT_col", b)
        ct = dict(ints=np.concatenate(tabs), where=where, foff=foff.tolist(), Ftot=Ftot, dev={})
        self._ct[key] = ct
        return ct

    def compact_device(self, depth: int, gates: int, device):
        """-> (tables dict, {key: device address}) of compact_tables on ``device`` (uploaded once)."""
        ct = self.compact_tables(depth, gates)
        device = torch.device(device)
        if device not in ct["dev"]:
            # (natively built tables live in the int32 pack the plan's own tables are views of: no second upload)
            d = self.to_device(device)["ints"] if ct.get("native") else F_.upload(ct["ints"], device)
            ct["dev"][device] = (d, None, {k: d.data_ptr() + 4 * off for k, (off, _) in ct["where"].items()})
        return ct, ct["dev"][device][2]

    def gate_rows(self, t: int, gates: int) -> np.ndarray:
        """Rows of the step's compact set inside the stacked [gates * E1, Hp] gate-input matrix."""
        off, n = self.where[("rows", t)]
        rows = self.ints[off:off + n].astype(np.int64)
        return np.concatenate([k * self.E1 + rows for k in range(gates)]).astype(np.int32)

    def to_device(self, device):
        """Device copies of the tables, one set PER DEVICE (kept for the life of the plan: the raw addresses handed to
        the C drivers -- ``ptr``, the cached ``ggpm_decode_steps`` descriptors under ``desc`` -- name exactly these
        tensors and live in the same dict, so they can never outlast them)."""
        device = torch.device(device)
        D = self._dev.get(device)
        if D is None and self._native is not None:
            sd = self._owner().to_device(device)._dev
            d64, d32 = sd["native"]
            nd = self._native.dir

            def view(name):
                pack, off, cnt, el = nd[name]
                return (d64 if pack == 1 else d32)[off // el:off // el + cnt]
            floff = nd["frozen_loc"][1]
            dl = d32.view(torch.uint8)[floff:floff + nd["frozen_loc"][2]]
            base = d32.data_ptr()
            ptr = {k: base + 4 * off for k, (off, n) in self.where.items()}
            meta = {k: dict(icls=view("meta_icls/%d" % k), nth=view("meta_nth/%d" % k), dest=view("meta_dest/%d" % k))
                    for k, _, _ in self.cand_blocks}
            D = self._dev[device] = dict(device=device, ints=d32, frozen_loc=dl, ptr=ptr, meta=meta, desc={}, seen=set(),
                                         pack64=d64)
        if D is None:
            di, dl = F_.upload(self.ints, device), F_.upload(self.frozen_loc, device)
            base = di.data_ptr()
            ptr = {k: base + 4 * off for k, (off, n) in self.where.items()}
            meta = {k: {n: F_.upload(v, device) for n, v in m.items()} for k, m in self.cand_meta.items()}
            for m in meta.values():
                m["icls"] = m["icls"].to(torch.int32)
            D = self._dev[device] = dict(device=device, ints=di, frozen_loc=dl, ptr=ptr, meta=meta, desc={}, seen=set())
        if device.type == "cuda":
            # uploaded on whatever stream was current then (the atom-ahead stream, usually) and read on others: tell the
            # allocator once per reading stream
            cur = torch.cuda.current_stream(device)
            if cur.cuda_stream not in D["seen"]:
                D["seen"].add(cur.cuda_stream)
                ts = [D["ints"], D["frozen_loc"]]
                ts +=[v for m in D["meta"].values() for v in m.values()] + ([D["pack64"]] if "pack64" in D else [])
                for t in ts:
                    t.record_stream(cur)
        return D


class DecodeSteps(ctypes.Structure):
    """include/ggpm_hip.h: ggpm_decode_steps (host arrays of per-step sizes / device pointers)."""
    _fields_ = [("T", ctypes.c_int), ("H", ctypes.c_int), ("depth", ctypes.c_int), ("lstm", ctypes.c_int),
                ("n", ctypes.c_void_p), ("foff", ctypes.c_void_p), ("roff", ctypes.c_void_p), ("qoff", ctypes.c_void_p),
                ("srcH", ctypes.c_void_p), ("srcF", ctypes.c_void_p), ("frozen", ctypes.c_void_p),
                ("pred_rowptr", ctypes.c_void_p), ("pred_col", ctypes.c_void_p), ("succ_rowptr", ctypes.c_void_p),
                ("succ_col", ctypes.c_void_p)]


def _decode_steps(plan: "AtomPlan", D, ct, cp, H: int, depth: int, lstm: bool):
    """The ggpm_decode_steps descriptor of (plan, device, depth, cell), built once (it only names resident tables)."""
    key = ("steps", depth, bool(lstm), H)
    hit = D["desc"].get(key)
    if hit is not None:
        return hit
    T, ptr = plan.T, D["ptr"]
    roff, qoff = plan.row_offsets(depth)
    arr32 = _lib.array_type(ctypes.c_int32, T)(*plan.nloc)
    a64 = lambda v: _lib.array_type(ctypes.c_int64, T + 1)(*[int(x) for x in v])
    pa = lambda vals: _lib.array_type(ctypes.c_void_p, T)(*[int(v) for v in vals])
    frz = D["frozen_loc"].data_ptr()
    keep = dict(n=arr32, foff=a64(ct["foff"]), roff=a64(roff), qoff=a64(qoff),
                srcH=pa(cp[("srcH", t)] for t in range(T)), srcF=pa(cp[("srcF", t)] for t in range(T)),
                frozen=pa(frz + plan.floc_off[t] for t in range(T)),
                pred_rowptr=pa(ptr[("lpred_rp", t)] for t in range(T)), pred_col=pa(ptr[("lpred_col", t)] for t in range(T)),
                succ_rowptr=pa(ptr[("lsucc_rp", t)] for t in range(T)), succ_col=pa(ptr[("lsucc_col", t)] for t in range(T)))
    d = DecodeSteps(T, H, depth, int(lstm), *[ctypes.addressof(keep[k]) for k in
                                               ("n", "foff", "roff", "qoff", "srcH", "srcF", "frozen", "pred_rowptr",
                                                "pred_col", "succ_rowptr", "succ_col")])
    D["desc"][key] = (d, keep)      # beside the tensors whose addresses it holds
    return d, keep


# The two step loops are ~280 launches = 1.5-1.8 ms of host time each, inside one C call (csrc/decode.hip; the weights are
# packed by the first step and shared by the others).  _dev.ATOM_ASYNC (default; read at CALL time, like every _dev
# setting) hands them to a worker thread of the library (ggpm_decode_steps_*_async): the forward loop is then issued
# beside the encoder's forward, the backward loop beside the encoder's backward -- the autograd engine reaches the two
# nodes at about the same time and would otherwise issue one chain only after the other, although they do not depend on
# each other.  What follows a loop on its stream (read-out / parameter gradients) is enqueued after ggpm_decode_join.
# Without it, and in a backward whose gradients cannot be published, the synchronous entry points issue the same launches
# from the calling thread.
_INFLIGHT: list = []         # buffers named by loops the worker may still be issuing (released by the next join)


def _join_worker(what: str) -> None:
    _lib.check(_lib.load().ggpm_decode_join(), what)
    del _INFLIGHT[:]


def _vp(addr: int) -> ctypes.c_void_p:
    return ctypes.c_void_p(addr)


def _cell(kind: str, params, I: int, H: int):
    """-> (the adapter of the message function, W_out, b_out) from the node's parameter tuple"""
    return F_.cell_for(kind == "LSTM", params[:-2], I, H), params[-2], params[-1]


def _compact_prelude(plan: AtomPlan, kind: str, depth: int, H: int, I: int, hmess, params):
    """What the training and the forward-only form do in front of their step loop: the hoisted gate input projections of
    ALL bond messages and the rows every step needs of them (gathered step by step into ``X_all``), the weight pack, the
    weight arrays and the descriptor of the decode driver.
    -> (device tables, cell, W_out, b_out, ct, cp, X_all, wpack, W_arr, ld_arr, desc, what desc names)"""
    dev = hmess.device
    D = plan.to_device(dev)
    cell, Wout, bout = _cell(kind, params, I, H)
    G, Hp, E1 = cell.G, cell.Hp, plan.E1
    ct, cp = plan.compact_device(depth, G, dev)
    f32 = dict(dtype=torch.float32, device=dev)
    X = torch.empty(G, E1, Hp, **f32)
    cell.project_inputs(hmess, F_._ld(hmess), E1, X)
    X_all = torch.empty(G * ct["Ftot"], Hp, **f32)
    _lib.check(_lib.load().ggpm_gather_rows(F_._p(X), Hp, _vp(cp["xrows"]), G * ct["Ftot"], Hp, F_._p(X_all), Hp, 0, 0,
                                            F_._stream()), "gather_rows")
    W_arr, ld_arr = cell.hidden_weight_arrays()
    desc, keep = _decode_steps(plan, D, ct, cp, H, depth, G == 4)
    return D, cell, Wout, bout, ct, cp, X_all, cell.alloc_pack(), W_arr, ld_arr, desc, keep


def _readout_stage(plan: AtomPlan, cp, state_src, agr_col, fn_all, Wout, bout, Fdim: int, H: int, drop, deferred: bool,
                   what: str):
    """Read-out of all steps at once: incoming messages (at their step's time) -> atoms -> clusters / candidates.
    ``state_src``: the buffer that holds every step's final states; ``agr_col``: the column array of the read-out CSR in that
    buffer's row numbering.  ``deferred``: the step loop is still being issued by the worker, so the read-out follows it
    after the join, in ``finish``.  -> (pooled, cand, NODE, NEI, finish or None)"""
    lib, P = _lib.load(), F_._p
    dev = fn_all.device
    f32 = dict(dtype=torch.float32, device=dev)
    Hp = F_.padded_hidden(H)
    ns_tot, n_inst = plan.aoff[-1], plan.ioff[-1]
    NEI = torch.empty(ns_tot, Hp, **f32)
    NODE = torch.empty(ns_tot, Hp, **f32)
    pooled = torch.empty(n_inst, Hp, **f32)
    cand = torch.empty(max(plan.n_cand, 1), Hp, **f32)
    ldF, ldwo = F_._ld(fn_all), Wout.stride(0)
    stream_obj = torch.cuda.current_stream(dev)

    def readout():
        s_ = F_._stream()
        _lib.check(lib.ggpm_segment_sum(P(state_src), Hp, _vp(cp["agr_rp"]), agr_col, ns_tot, H, P(NEI), Hp, 0, Hp, s_),
                   "segment_sum")
        F_.gemm_ksegments(1, ns_tot, H, [fn_all, NEI], [ldF, Hp], [Wout, Wout[:, Fdim:]], [ldwo, ldwo], [Fdim, H], NODE, Hp,
                          Hp, bias=bout, act=F_.ACT_RELU)
        if drop is not None:
            _lib.check(lib.ggpm_dropout(P(NODE), ns_tot, H, Hp, drop[0], drop[1], drop[2], 0, s_), "dropout")
        _lib.check(lib.ggpm_segment_sum(P(NODE), Hp, _vp(cp["pool_rp"]), _vp(cp["pool_col"]), n_inst, H, P(pooled), Hp, 0, Hp,
                                        s_), "segment_sum")
        _lib.check(lib.ggpm_gather_rows(P(NODE), Hp, _vp(cp["cand_idx"]), max(plan.n_cand, 1), H, P(cand), Hp, 0, Hp, s_),
                   "gather_rows")

    def finish():
        _join_worker(what)
        with torch.cuda.stream(stream_obj):
            readout()

    if not deferred:
        readout()
    return pooled, cand, NODE, NEI, (finish if deferred else None)


class _AtomDecodeCompact(torch.autograd.Function):
    """(pooled cluster vectors of all visits [n_inst, Hp], attachment-candidate atom vectors [n_cand, Hp]) from decode steps
    on compact row sets (module docstring, ``AtomPlan.compact_tables``): inside the step loop only ``gather frozen rows ->
    sparse_forward`` (backward: ``sparse_backward -> scatter-add to the rows' sources``); gate inputs of all steps gathered
    once, read-out of all steps batched behind the loop, weight gradients contracted once over the stacked stashes."""

    @staticmethod
    def launch(plan: AtomPlan, kind: str, depth: int, H: int, Fdim: int, I: int, fn_all, hmess, drop, params,
               infer: bool = False) -> dict:
        """Everything the forward computes, issued now (no autograd node): -> state for ``forward(..., state, *params)``.
        ``HierMPNDecoder.start_atom_level`` calls this BEFORE the encoder runs and creates the node later, behind the
        encoder's: the engine then reaches this node first in the backward pass and -- its loop being issued by the worker
        thread -- goes straight on to the encoder's backward, so that the longer chain starts first.
        ``infer``: the forward-only form (no backward follows; no autograd node is made): every step's depth loop runs in
        ping-pong scratch and only the final state of its rows is kept, at its F ids (ggpm_decode_steps_infer) -- no
        Hs_all / Qs_all / St_all; the read-out reads those rows (``_agr_f_col``).  Same launches, same outputs."""
        if infer:
            return _launch_infer(plan, kind, depth, H, Fdim, I, fn_all, hmess, drop, params)
        lib, P = _lib.load(), F_._p
        D, cell, Wout, bout, ct, cp, X_all, wpack, W_arr, ld_arr, desc, _keep = _compact_prelude(plan, kind, depth, H, I, hmess,
                                                                                                params)
        Hp, lstm = cell.Hp, cell.G == 4
        f32 = dict(dtype=torch.float32, device=hmess.device)
        roff, qoff = plan.row_offsets(depth)
        Hs_all = torch.empty(qoff[-1], Hp, **f32)
        Cs_all = torch.empty(qoff[-1], Hp, **f32) if lstm else None
        Qs_all = torch.empty(roff[-1], Hp, **f32)
        St_all = torch.empty(5, roff[-1], Hp, **f32)
        # the whole step loop as one C call (csrc/decode.hip)
        tmp = torch.empty(2 * max(plan.nloc), Hp, **f32)
        deferred = _dev.ATOM_ASYNC
        fn = lib.ggpm_decode_steps_forward_async if deferred else lib.ggpm_decode_steps_forward
        _lib.check(fn(
            ctypes.byref(desc), W_arr, ld_arr, P(cell.b_u), P(X_all), P(Hs_all), P(Cs_all), P(Qs_all), P(St_all),
            St_all.stride(0), P(wpack), P(tmp), F_._stream()), "decode_steps_forward")
        if deferred:
            _INFLIGHT.append((desc, _keep, X_all, Hs_all, Cs_all, Qs_all, St_all, wpack, tmp, params))
        pooled, cand, NODE, NEI, finish = _readout_stage(plan, cp, Hs_all, _vp(cp["agr_col"]), fn_all, Wout, bout, Fdim, H, drop,
                                                         deferred, "decode_join (forward)")
        return dict(pooled=pooled, cand=cand, finish=finish, keep=(D, ct, cp),
                    saved=(fn_all, hmess, NODE, NEI, X_all, Hs_all, Qs_all, St_all) + ((Cs_all,) if lstm else ()))

    @staticmethod
    def forward(ctx, plan: AtomPlan, cell: str, depth: int, H: int, Fdim: int, I: int, fn_all, hmess, drop, state, *params):
        ctx.plan, ctx.meta, ctx.drop = plan, (cell, depth, H, Fdim, I), drop
        ctx.save_for_backward(*state["saved"], *params)
        ctx.keep = state["keep"]
        ctx.params_ref = params            # the Parameter objects themselves (the async backward assigns their .grad)
        return state["pooled"], state["cand"]

    @staticmethod
    def backward(ctx, d_pooled, d_cand):
        lib = _lib.load()
        # everything upstream of the atom level (heads, the two tree-side levels) has run its backward: their queued
        # weight-gradient contractions can start beside this node and the encoder's backward.  They are ~45 launches of
        # host time: with the step loop handed to the worker thread they are issued AFTER the loop has been posted (below),
        # so that the longest chain of the pass starts first; without the worker, here.
        F_.mark("bwd: atom level's node reached")
        flush_after_post = _dev.ATOM_ASYNC
        if not flush_after_post:
            F_.flush_deferred_early()
        plan, (kind, depth, H, Fdim, I), drop = ctx.plan, ctx.meta, ctx.drop
        lstm = kind == "LSTM"
        sv = list(ctx.saved_tensors)
        fn_all, hmess, NODE, NEI, X_all, Hs_all, Qs_all, St_all = sv[:8]
        Cs_all = sv[8] if lstm else None
        params = sv[9:] if lstm else sv[8:]
        cell, Wout, _ = _cell(kind, params, I, H)
        D, ct, cp = ctx.keep
        P = F_._p
        dev = hmess.device
        Hp = F_.padded_hidden(H)
        E1, G = plan.E1, cell.G
        f32 = dict(dtype=torch.float32, device=dev)
        d_pooled, d_cand = d_pooled.contiguous(), d_cand.contiguous()
        s = F_._stream()
        Ftot = ct["Ftot"]
        roff, qoff = plan.row_offsets(depth)
        ns_tot, ldwo = plan.aoff[-1], Wout.stride(0)
        # ---- read-out of all steps, backwards: clusters / candidates -> atoms -> the final states they read
        d_node = torch.empty(ns_tot, Hp, **f32)
        _lib.check(lib.ggpm_segment_sum(P(d_pooled), Hp, _vp(cp["poolT_rp"]), _vp(cp["poolT_col"]), ns_tot, H, P(d_node), Hp, 0,
                                        Hp, s), "segment_sum")
        if plan.n_cand > 0:
            _lib.check(lib.ggpm_segment_sum(P(d_cand), Hp, _vp(cp["candT_rp"]), _vp(cp["candT_col"]), ns_tot, H, P(d_node), Hp,
                                            1, 0, s), "segment_sum")
        DPRE = torch.empty(ns_tot, Hp, **f32)
        _lib.check(lib.ggpm_act_backward(P(d_node), P(NODE), ns_tot, H, Hp, F_.ACT_RELU, 0, P(DPRE), s), "act_backward")
        if drop is not None:                # d(dropout . relu) = mask * scale * relu' (the saved output is the dropped one)
            _lib.check(lib.ggpm_dropout(P(DPRE), ns_tot, H, Hp, drop[0], drop[1], drop[2], 0, s), "dropout")
        d_nei = torch.empty(ns_tot, Hp, **f32)
        F_.gemm(0, 0, ns_tot, H, H, DPRE, Hp, Wout[:, Fdim:], ldwo, d_nei, Hp, Hp)
        dF = torch.empty(Ftot, Hp, **f32)            # gradient of every step's final states (zero where nothing reads them)
        _lib.check(lib.ggpm_segment_sum(P(d_nei), Hp, _vp(cp["agrT_rp"]), _vp(cp["agrT_col"]), Ftot, H, P(dF), Hp, 0, Hp, s),
                   "segment_sum")
        dCF = torch.zeros(Ftot, Hp, **f32) if lstm else None
        dX_all = torch.empty(G * Ftot, Hp, **f32)
        # gate-gradient stashes of all steps, stacked like the forward's (DQ with a zero slot per step at the end so that it
        # lines up with the depth + 1 state slots): contracted once behind the loop
        DG_all = torch.empty(3 if lstm else 2, roff[-1], Hp, **f32)
        DQ_all = torch.zeros(qoff[-1], Hp, **f32)
        # the [H, I + H] gradient buffers of the gate weights exist from the start: the stacked contractions write their
        # hidden halves (``acc``; GRU: Wz_h, U_r, Wh_h, b_u) in place (leading dimension I + H), the grouped input-half launch
        # fills the rest -- no copies
        bufs, acc = cell.dW_buffers()
        nmax = max(plan.nloc)
        work = cell.backward_workspace(nmax, depth)
        params_ref = ctx.params_ref
        go_async = _dev.ATOM_ASYNC and F_.can_publish(*params_ref) and all(ctx.needs_input_grad[10:])
        # the whole step loop as one C call (csrc/decode.hip): per step sparse_backward, its stashes to the stacked buffers
        # (contracted once in tail()), the frozen rows' gradient scatter-added to the step that produced their state
        W_arr, ld_arr = cell.hidden_weight_arrays()
        desc, _keep = _decode_steps(plan, D, ct, cp, H, depth, lstm)
        tmp = torch.empty(2 * nmax, Hp, **f32)
        dW_arr = _lib.array_type(ctypes.c_void_p, 4)(*[a.data_ptr() for a in acc])
        fn = lib.ggpm_decode_steps_backward_async if go_async else lib.ggpm_decode_steps_backward
        _lib.check(fn(
            ctypes.byref(desc), W_arr, ld_arr, P(X_all), P(Hs_all), P(Cs_all), P(Qs_all), P(St_all), St_all.stride(0),
            P(dF), P(dCF), P(dX_all), P(DG_all), DG_all.stride(0), P(DQ_all), dW_arr, P(work), work.numel() * 4, P(tmp),
            s), "decode_steps_backward")
        if go_async:
            _INFLIGHT.append((desc, _keep, sv, dF, dCF, dX_all, DG_all, DQ_all, acc, work, tmp))
        F_.mark("bwd: atom loop posted")
        if flush_after_post:
            F_.flush_deferred_early()
        F_.mark("bwd: atom node returns")
        # ---- parameter gradients, once
        def tail():
            s_ = F_._stream()
            dX_tot = torch.empty(G, E1, Hp, **f32)
            _lib.check(lib.ggpm_segment_sum(P(dX_all), Hp, _vp(cp["xT_rp"]), _vp(cp["xT_col"]), G * E1, Hp, P(dX_tot), Hp, 0, 0, s_),
                       "segment_sum")
            R, RQ = roff[-1], qoff[-1]
            wsb = int(lib.ggpm_weight_grads_stacked_workspace_bytes(H, max(R, RQ)))
            ws = torch.empty((wsb + 3) // 4, **f32)
            ld = [a.stride(0) for a in acc[:G]]
            if lstm:        # acc: Wi_h, Wo_h, Wu_h, Wf_h; St_all[0] = S
                _lib.check(lib.ggpm_lstm_weight_grads_stacked(
                    R, RQ, H, P(DG_all[0]), P(DG_all[1]), P(DG_all[2]), P(St_all[0]), P(DQ_all), P(Hs_all), P(acc[0]), ld[0],
                    P(acc[1]), ld[1], P(acc[2]), ld[2], P(acc[3]), ld[3], P(ws), ws.numel() * 4, s_), "lstm_weight_grads_stacked")
            else:           # acc: Wz_h, U_r, Wh_h, b_u; St_all: S, G, Z, M, R
                _lib.check(lib.ggpm_gru_weight_grads_stacked(
                    R, RQ, H, P(DG_all[0]), P(St_all[1]), P(DG_all[1]), P(St_all[0]), P(DQ_all), P(Hs_all), P(acc[0]), ld[0],
                    P(acc[1]), ld[1], P(acc[3]), P(acc[2]), ld[2], P(ws), ws.numel() * 4, s_), "gru_weight_grads_stacked")
            return _param_grads(cell, Wout, acc, dX_tot, hmess, DPRE, NEI, fn_all, Fdim, E1, ns_tot, bufs)

        if go_async:
            # The loop is being issued by the worker; this node returns now so that the engine can issue the encoder's
            # backward beside it.  At the end of the pass: join the worker, enqueue the tail behind the loop on the atom
            # level's stream, hand the gradients to .grad on the stream the rest of the step consumes them on.
            atom_stream = torch.cuda.current_stream(dev)

            def finish():
                F_.mark("bwd: end-of-pass callback")
                _join_worker("decode_join (backward)")
                main = torch.cuda.current_stream(dev)
                with torch.cuda.stream(atom_stream):
                    F_.mark("bwd: atom loop done (its stream)")
                    grads = tail()
                    F_.mark("bwd: atom level's tail issued")
                main.wait_stream(atom_stream)
                for prm, g in zip(params_ref, grads):
                    F_._accumulate_grad(prm, g, main)
            torch.autograd.Variable._execution_engine.queue_callback(finish)
            return (None,) * (10 + len(params))
        return (None,) * 10 + tail()


def _agr_f_col(plan: AtomPlan, ct: dict, depth: int, device) -> torch.Tensor:
    """The read-out CSR's columns (``agr_col``: rows of the stacked [(depth + 1) * n_t] state blocks) as F ids, i.e. rows
    of the forward-only form's final-state buffer, in the same order (cached per device)."""
    key = ("agrF", torch.device(device))
    hit = ct.get(key)
    if hit is not None:
        return hit
    n = np.asarray(plan.nloc, dtype=np.int64)
    foff = np.asarray(ct["foff"], dtype=np.int64)
    qoff = np.concatenate([[0], np.cumsum((depth + 1) * n)])
    h2f = np.full(int(qoff[-1]), -1, dtype=np.int64)
    for t in range(plan.T):
        base = qoff[t] + depth * n[t]
        h2f[base:base + n[t]] = foff[t] + np.arange(n[t])
    d = ct["dev"][torch.device(device)][0]
    off, ln = ct["where"]["agr_col"]
    col = torch.from_numpy(h2f).to(device)[d[off:off + ln].long()].to(torch.int32).contiguous()
    ct[key] = col
    return col


def _launch_infer(plan: AtomPlan, kind: str, depth: int, H: int, Fdim: int, I: int, fn_all, hmess, drop, params) -> dict:
    """The forward-only form of ``_AtomDecodeCompact.launch`` (see there)."""
    lib, P = _lib.load(), F_._p
    params = tuple(p.detach() for p in params)
    _, cell, Wout, bout, ct, cp, X_all, wpack, W_arr, ld_arr, desc, _keep = _compact_prelude(plan, kind, depth, H, I, hmess, params)
    Hp, lstm, Ftot = cell.Hp, cell.G == 4, ct["Ftot"]
    f32 = dict(dtype=torch.float32, device=hmess.device)
    agr_col = _agr_f_col(plan, ct, depth, hmess.device)
    F_h = torch.empty(max(Ftot, 1), Hp, **f32)              # final state of every step's rows, by F id
    F_c = torch.empty(max(Ftot, 1), Hp, **f32) if lstm else None
    Hs, Cs, Qs, _ = cell.alloc_state(max(plan.nloc), depth, save=False)        # ping-pong scratch of the largest step
    deferred = _dev.ATOM_ASYNC
    fn = lib.ggpm_decode_steps_infer_async if deferred else lib.ggpm_decode_steps_infer
    _lib.check(fn(ctypes.byref(desc), W_arr, ld_arr, P(cell.b_u), P(X_all), P(F_h), P(F_c), P(Hs), P(Cs), P(Qs), P(wpack),
                  F_._stream()), "decode_steps_infer")
    if deferred:
        _INFLIGHT.append((desc, _keep, X_all, F_h, F_c, Hs, Cs, Qs, wpack, params))
    pooled, cand, _, _, finish = _readout_stage(plan, cp, F_h, P(agr_col), fn_all, Wout, bout, Fdim, H, drop, deferred,
                                                "decode_join (forward-only)")
    return dict(pooled=pooled, cand=cand, finish=finish)


def _param_grads(cell, Wout, acc, dX_tot, hmess, DPRE, NEI, fn_all, Fdim, E1, ns_tot, bufs):
    """Parameter gradients of the atom-level decode from the summed gate-input gradients, the hidden halves ``acc`` and the
    stacked read-out rows.  ``bufs``: the gate weights' gradient buffers, whose hidden halves ``acc`` are (written in
    place by the stacked contractions)."""
    H, Hp, I = cell.H, cell.Hp, cell.I
    # input halves dW_k[:, :I] = dX_k^T hmess of all gates in ONE grouped launch (as the encoder's drivers form them)
    F_.gemm_grouped(1, 0, H, I, E1, [dict(A=dX_tot[k], lda=Hp, B=hmess, ldb=F_._ld(hmess), C=b, ldc=b.stride(0), n_pad=I)
                                      for k, b in enumerate(bufs)], splitk=True)
    dWout = torch.empty_like(Wout)
    F_.gemm(1, 0, H, Fdim, ns_tot, DPRE, Hp, fn_all, F_._ld(fn_all), dWout, dWout.stride(0), Fdim, splitk=True)
    F_.gemm(1, 0, H, H, ns_tot, DPRE, Hp, NEI, Hp, dWout[:, Fdim:], dWout.stride(0), H, splitk=True)
    dbout = F_.colsum(DPRE, ns_tot, H)
    dbs = [F_.colsum(dX_tot[k], E1, H) if b is not None else None for k, (_, b) in enumerate(cell.gates)]      # gate biases
    return cell.grads(bufs, acc, dbs) + (dWout, dbout)


class AtomRun:
    """One issued atom level: its launch stream, its two result tensors and what is still owed on them -- ``finish`` (the
    worker's join and the read-out behind the step loop, or None) and ``node`` = (args, state, params) of the
    ``_AtomDecodeCompact`` node where autograd records (None for the forward-only form, which makes no node)."""

    def __init__(self, stream, pooled, cand, finish=None, node=None):
        self.stream, self.pooled, self.cand = stream, pooled, cand
        self._finish, self._node = finish, node

    def join(self):
        """-> (pooled, cand), ready for the launch stream's next reader.  The first call pays what is owed, inside the
        launch stream (the node's backward runs on the stream of its forward), and drops the closure and the state."""
        finish, node = self._finish, self._node
        self._finish = self._node = None
        if finish is not None or node is not None:
            with torch.cuda.stream(self.stream):
                if finish is not None:
                    finish()
                if node is not None:
                    args, state, params = node
                    self.pooled, self.cand = _AtomDecodeCompact.apply(*args, state, *params)
        return self.pooled, self.cand


def atom_decode_launch(plan: AtomPlan, graph_encoder, hnode_a: torch.Tensor, hmess_a: torch.Tensor,
                       fn_all: torch.Tensor) -> AtomRun:
    """Issues the atom level of ``graph_encoder`` = the decoder's atom-level ``IncMPNEncoder`` on the current stream.
    With _dev.ATOM_ASYNC the step loop is still being issued by a worker thread when this returns: ``AtomRun.join``
    comes before anything reads the two tensors or another stream waits on this one."""
    from .rnn import LSTM
    rnn, wo = graph_encoder.rnn, graph_encoder.W_o
    lstm, params = isinstance(rnn, LSTM), rnn.level_params()
    drop = None
    if graph_encoder.training and wo[2].p > 0:
        seed = getattr(graph_encoder, "_dropout_seed", None)           # (tests pin the seed)
        if not seed:
            seed = torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int64)
        drop = (float(wo[2].p), int(seed[0]), int(seed[1]))
    args =(plan, "LSTM" if lstm else "GRU", rnn.depth, rnn.hidden_size, graph_encoder.node_fdim, rnn.input_size, fn_all,
            hmess_a, drop)
    params = params + (wo[0].weight, wo[0].bias)
    # a call autograd will not record runs the forward-only form, which makes no node: once joined, nothing of it is left
    # in _INFLIGHT for a backward to collect
    infer = not fused.records_grad(params + (fn_all, hmess_a))
    stream = torch.cuda.current_stream(hmess_a.device)
    with torch.no_grad():
        state = _AtomDecodeCompact.launch(*args, params, infer=infer)
    return AtomRun(stream, state["pooled"], state["cand"], state.pop("finish"), None if infer else (args, state, params))


def atom_decode(plan: AtomPlan, graph_encoder, hnode_a: torch.Tensor, hmess_a: torch.Tensor, fn_all: torch.Tensor):
    """-> (pooled [n_inst, Hp], cand [n_cand, Hp]): ``atom_decode_launch`` joined at once."""
    return atom_decode_launch(plan, graph_encoder, hnode_a, hmess_a, fn_all).join()
