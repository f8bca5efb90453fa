"""
GPU (-m gpu): a result may depend only on the logical operand -- never on its address, never on its surroundings.

Every entry point below runs once on aligned, unpadded clones of its operands (the control) and then once per placement
(tests/placement.py): one operand at a time
    * at every element offset that leaves the 16-byte grid (fp32 / int32: 1 2 3, fp64: 1, fp16: 1 .. 7) -- the pointer half of the
      loaders' `ld % m == 0 && stride % m == 0 && (uintptr_t)p % 16 == 0` dispatch, and, displaced singly, each side of the
      OR-ed `A | Bm` forms;
    * as pairs 1: of a batch one larger (what shard.py hands a rank);
    * (eigenvector arrays) at row strides k + 1 and k + 5 with the columns behind k -- and the memory in front of and behind the
      array -- filled with NaN, +Inf, -Inf, half the largest finite value, the smallest subnormal; once with an offset as well;
    * (operands without padding: maps, projected descriptors, spectra, masses, cost matrices, point sets) with each of the five fills
      in the guards in front of and behind the array;
    * (padded batches: fps, signatures, lsa_gather, groups_dmtx, map_accuracy / map_continuity / map_coverage) as meshes of n_verts
      vertices in arrays of n_verts + 1 and n_verts + 5 rows -- for the distance matrices also columns -- with every fill behind
      n_verts.  Their index lists are ragged host lists that the engine checks against n_verts before a launch: no index padding;
then all operands displaced together.  Each run is compared with
    (a) the float64 oracle of the operation, at the tolerance the entry's existing test uses (cited in tests/placement_cases.py
        next to each bound), and
    (b) the control: integer outputs identical, floating outputs BIT-identical.
The placed pointer is checked to be what the library received (a recording shim around the ctypes entry), not assumed.

Held to (a) only, not to bits:
    * project / fmap_fit with proj_onepass = 1 and fp16 descriptors that start at an odd element (offsets 1 3 5 7): the one-pass
      kernel reads descriptor rows with dword-granular 16-byte buffer loads, so dm_project_f16split_launch (dm_project.hip,
      `onepass_ok`) sends descriptors that are not on a dword boundary to the two-launch kernels instead; the two kernels scale
      and accumulate differently (tests/test_gpu_project.py compares them at 2e-6, not to bits).
Everything else is held to bits: the loader pairs of dm_gemm_f64.h, dm_p2p.hip, dm_knnsplit.hip and dm_project.hip differ only in
how the operands are fetched (PartPair::sum equals operator double when the second chunk is absent, a maximum is order-free).

dm_simnn_f16 refuses fp16 features that are not 16-byte aligned: the refusal, that nothing was launched, and an aligned call
afterwards are asserted instead.
"""
import numpy as np
import pytest
import torch

import placement as pl
import placement_cases as pc
from oracle import dm_oracle as orc

pytestmark = pytest.mark.gpu

LD_EXTRA = pc.LD_EXTRA


@pytest.fixture(scope="module")
def _engine():
    from densematcher_amd.engine import MatchEngine
    return MatchEngine()


@pytest.fixture
def eng(_engine):
    """the module's engine; code-path options (dm_set_option) are back at their defaults after every test"""
    yield _engine
    _engine.reset_options()


def _np(out):
    return {n: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for n, v in out.items() if v is not None}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _variants(entry, ops):
    """(name, {operand: place() keywords}) -- one operand at a time, then all together"""
    out = []
    for name, arr in ops.items():
        t = torch.as_tensor(arr)
        wide = tuple(arr.shape[-1] + e for e in LD_EXTRA) if name in entry.ld_of else ()
        tall = tuple(arr.shape[-2] + e for e in LD_EXTRA) if name in entry.rows_only else ()
        geom = dict(squares=wide) if name in entry.rows_of else dict(lds=wide, rows=tall)
        out += [(f"{name}:{pn}", {name: kw}) for pn, kw in pl.placements(t.dtype, batch=arr.ndim >= 2, **geom)]
    together = {}
    for name, arr in ops.items():
        t = torch.as_tensor(arr)
        together[name] = dict(offset_elems=pl.OFFSETS[t.dtype][0])
        if name in entry.ld_of:
            together[name].update(ld=arr.shape[-1] + LD_EXTRA[-1], pad="-inf")
        if name in entry.rows_of or name in entry.rows_only:
            together[name].update(rows=arr.shape[-2] + LD_EXTRA[-1], pad="-inf")
    out.append(("all:off+ld/-inf", together))
    out.append(("all:slice", {name: dict(slice_of_batch=True) for name, arr in ops.items() if arr.ndim >= 2}))
    return out


@pytest.mark.parametrize("case", pc.all_cases(), ids=pc.case_id)
def test_placement(eng, case):
    entry, cfg = case
    ops = entry.build(cfg)
    ref = entry.oracle(ops, cfg)
    dev = eng.device
    control_ops = {n: pl.place(a, device=dev).clone() for n, a in ops.items()}
    assert all(t.data_ptr() % 16 == 0 for t in control_ops.values())
    control = _np(entry.call(eng, control_ops, cfg))
    msg = entry.check(control, ref, cfg)
    assert msg is None, f"control (aligned, unpadded): {msg}"
    failures = []
    for vname, moved in _variants(entry, ops):
        T = dict(control_ops)
        for name, kw in moved.items():
            T[name] = pl.place(ops[name], device=dev, **kw)
        with pl.PointerRecorder(eng.lib, entry.lib(cfg)) as rec:
            got = _np(entry.call(eng, T, cfg))
        assert rec.saw(*[T[n] for n in moved]), f"{vname}: the library did not receive the placed pointers"
        msg = entry.check(got, ref, cfg)
        if msg is not None:
            failures.append(f"{vname}: oracle: {msg}")
        for n, g in got.items():
            exact = np.issubdtype(g.dtype, np.integer) or not entry.loose(cfg, moved)
            if exact and not _same_bits(g, control[n]):
                d = (g != control[n])
                failures.append(f"{vname}: {n} differs from the control in {int(d.sum())} of {d.size} entries"
                                + ("" if np.issubdtype(g.dtype, np.integer) else f" (max |diff| {np.nanmax(np.abs(g.astype(np.float64) - control[n])):.3e})"))
    assert not failures, f"{len(failures)} placement(s) change the result:\n  " + "\n  ".join(failures)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [24, 40])
def test_simnn_refuses_unaligned_features(eng, D):
    """dm_simnn_f16 takes 16-byte fp16 rows: a feature pointer off the 16-byte grid is refused with the documented message before
    anything is launched; the same engine then answers an aligned call with the oracle's map; batch slices of features with
    D % 8 == 0 are aligned by construction, are accepted and equal the control"""
    rng = np.random.default_rng(D)
    Ft = rng.standard_normal((pc.B, pc.N2, D)).astype(np.float16)
    Fs = rng.standard_normal((pc.B, pc.N1, D)).astype(np.float16)
    ref = np.stack([orc.simnn(Ft[b], Fs[b]) for b in range(pc.B)])
    ct, cs = pl.place(Ft, device=eng.device), pl.place(Fs, device=eng.device)
    control = eng.simnn(ct, cs).cpu().numpy()
    assert np.array_equal(control, ref)
    for off in pl.OFFSETS[torch.float16]:
        for which in ("tgt", "src", "both"):
            T = pl.place(Ft, device=eng.device, offset_elems=off, pad="+inf") if which != "src" else ct
            S = pl.place(Fs, device=eng.device, offset_elems=off, pad="+inf") if which != "tgt" else cs
            eng.profile_kernel("*")
            try:
                with pl.PointerRecorder(eng.lib, "dm_simnn_f16") as rec:
                    with pytest.raises(ValueError, match="feature pointers must be 16-byte aligned"):
                        eng.simnn(T, S)
                assert rec.saw(T, S)
                assert eng.profile_report() == {}, "a refused call launched kernels"
            finally:
                eng.profile_kernel("")
    assert np.array_equal(eng.simnn(ct, cs).cpu().numpy(), ref)
    for pad in pl.PADS:
        T = pl.place(Ft, device=eng.device, slice_of_batch=True, pad=pad)
        S = pl.place(Fs, device=eng.device, slice_of_batch=True, pad=pad)
        assert T.data_ptr() % 16 == 0 and S.data_ptr() % 16 == 0
        with pl.PointerRecorder(eng.lib, "dm_simnn_f16") as rec:
            got = eng.simnn(T, S).cpu().numpy()
        assert rec.saw(T, S) and np.array_equal(got, control), pad
