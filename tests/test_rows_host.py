"""Rows by id, the parts that need no GPU: the fourth header and its exports, the cases of tests/rows_cases.py against NumPy
forms of the kernels -- the right one passes every case, and each wrong one (ids cut to 32 bits, the wrong pitch, leaked
padding columns, arithmetic instead of a bit copy, a pairwise sum, L2 answered as inner product) fails at least one, i.e. the
GPU tests of tests/test_gpu_rows.py can fail --, the formula of the shim's L2 column, and ShardedMipsIndex.reconstruct_batch on
gloo ranks with an injected local step."""
import os
import re
import sys

import numpy as np
import pytest

import retrieval_augmented_mds_amd as ram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import rows_cases as rc
finally:
    sys.path.pop(0)


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return text, set(re.findall(r"\b(mips_[a-z0-9_]+)\s*\(", text))


# ------------------------------------------------------------------ 1. ABI pins
def test_fourth_header_declares_and_library_exports_the_row_calls():
    text, declared = _declared(os.path.join(ROOT, "include", "mips_hip_rows.h"))
    assert '#include "mips_hip.h"' in text and "MIPS_ABI_VERSION" not in text
    assert set(ram._lib.EXPORTS_ROWS) == declared == {"mips_index_reconstruct", "mips_index_gather_labels", "mips_score_subset"}
    old = set()
    for name in ("mips_hip.h", "mips_hip_update.h", "mips_hip_sharded.h"):
        old |= _declared(os.path.join(ROOT, "include", name))[1]
    assert not declared & old
    assert set(ram._lib.EXPORTS) | set(ram._lib.EXPORTS_UPDATE) | set(ram._lib.EXPORTS_SHARDED) == old
    # the new flags use bits of their own
    assert re.search(r"#define MIPS_IDS_DEVICE 64\b", text) and re.search(r"#define MIPS_ROWS_ZERO_MISSING 128\b", text)
    assert (ram._lib.IDS_DEVICE, ram._lib.ROWS_ZERO_MISSING) == (64, 128)
    used = ram._lib.Q_DEVICE | ram._lib.OUT_DEVICE | ram._lib.OUT_PACKED | ram._lib.FORCE_IP | ram._lib.SEL_DEVICE | ram._lib.GRP_DEVICE
    assert used & (64 | 128) == 0
    lib = ram._lib.load()                                                          # builds, loads and binds
    assert len(lib.mips_index_reconstruct.argtypes) == 9 and len(lib.mips_index_gather_labels.argtypes) == 7
    assert len(lib.mips_score_subset.argtypes) == 10
    assert ram._lib.HEADER_ROWS in ram._lib._sources()                             # a change of the header rebuilds the library
    for name in ("rows_kernels.hpp", "host_rows.hpp"):
        assert os.path.join(ram._lib.CSRC, name) in ram._lib._sources()


def test_python_surface():
    import inspect

    for name in ("reconstruct", "reconstruct_n", "reconstruct_batch", "search_and_reconstruct", "compute_distance_subset", "labels_of"):
        assert hasattr(ram.MipsIndex, name), name
    for name in ("reconstruct", "reconstruct_n", "reconstruct_batch", "search_and_reconstruct", "compute_distance_subset"):
        assert hasattr(ram.faiss_shim.IndexFlat, name), name
    p = inspect.signature(ram.MipsIndex.reconstruct_batch).parameters
    assert (p["raw"].default, p["idx_offset"].default, p["out"].default) == (False, 0, None)
    assert "local_reconstruct" in inspect.signature(ram.ShardedMipsIndex.__init__).parameters
    assert inspect.signature(ram.Mips.search_device).parameters["return_rows"].default is False
    assert hasattr(ram.Mips, "retrieved_group_hits")


def test_host_ids_are_int64_or_refused():
    import types

    me = types.SimpleNamespace(device=0)                                           # (the NumPy branch reads nothing of the index)
    ptr, shape, is_dev, keep = ram.MipsIndex._ids_arg(me, np.array([[1, 2]], np.uint64), "t")
    assert shape == (1, 2) and not is_dev and keep.dtype == np.int64 and keep.tolist() == [[1, 2]]
    with pytest.raises(ValueError, match="int64"):
        ram.MipsIndex._ids_arg(me, np.array([1 << 63], np.uint64), "t")            # would wrap to a negative id: "no row"
    with pytest.raises(ValueError, match="integer"):
        ram.MipsIndex._ids_arg(me, np.array([1.0]), "t")
    assert ram.MipsIndex._ids_arg(me, [], "t")[1] == (0,)


def test_kernels_are_not_scan_kernels():
    import scan_recipes as sr

    text = open(os.path.join(ram._lib.CSRC, "rows_kernels.hpp")).read()
    names = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", text)
    assert sorted(names) == ["rows_gather_kernel", "rows_gather_labels_kernel", "rows_score_kernel"]
    assert not any(("mips::" + n).startswith(sr.SCAN_PREFIXES) for n in names)


def test_pitch_model_is_the_library_rule():
    assert [rc.pitch_of("bf16", d) for d in rc.DIMS] == [128, 128, 128, 128, 768, 1024, 1024, 1536]
    assert [rc.pitch_of("f32", d) for d in rc.DIMS] == [64, 64, 64, 128, 768, 832, 1024, 1536]
    assert [rc.pitch_of("fp8_e4m3", d) for d in rc.dims_of("fp8_e4m3")] == [256, 256, 256, 256, 768, 1024, 1024]


# ------------------------------------------------------------------ 2. the cases reject wrong kernels
def _reconstruct_failures(mutant):
    """Names of the cases a NumPy kernel (right: mutant None) gets wrong."""
    bad = []
    shapes = [("bf16", 7, 129), ("bf16", 100, 129), ("fp8_e4m3", 100, 127), ("f32", 100, 129), ("bf16", 1, 1)]
    for storage, d, n in shapes:
        x = rc.planted_f32(n, d) if storage == "f32" else rc.rows_data(storage, d, n)[1]
        img = rc.storage_image(x, rc.pitch_of(storage, d))
        for name, ids in rc.id_patterns(n).items():
            for off, zero in ((0, False), (1000, False), (n // 2, True)):
                for out_ld in (d, d + 3):
                    out = np.full((len(ids), out_ld), rc.SENTINEL, np.uint32)
                    rc.kernel_reconstruct(img, d, ids + off if off != n // 2 else ids, off, out, zero, mutant)
                    exp = rc.model_reconstruct(x, ids + off if off != n // 2 else ids, off, zero).view(np.uint32)
                    if not (np.array_equal(out[:, :d], exp) and np.all(out[:, d:] == rc.SENTINEL)):
                        bad.append(f"{storage}-d{d}-n{n}-{name}-off{off}-ld{out_ld}")
    return bad


def test_the_right_gather_passes_every_case():
    assert _reconstruct_failures(None) == []


@pytest.mark.parametrize("mutant,must_fail", [("ids_int32", "bad_two32_plus_3"), ("pitch_d", "identity"), ("leak_padding", "-ld"),
                                              ("float_add", "f32-")])
def test_a_wrong_gather_fails_a_case(mutant, must_fail):
    bad = _reconstruct_failures(mutant)
    assert bad and any(must_fail in b for b in bad), (mutant, bad[:5])


def test_float_add_loses_exactly_the_planted_minus_zero():
    x = rc.planted_f32()
    img = rc.storage_image(x, rc.pitch_of("f32", x.shape[1]))
    ids = np.arange(len(x), dtype=np.int64)
    out = rc.kernel_reconstruct(img, x.shape[1], ids, 0, np.zeros(x.shape, np.uint32), mutant="float_add")
    diff = out != x.view(np.uint32)
    assert diff.any() and np.all(x.view(np.uint32)[diff] == 0x80000000)


def _score_cases():
    x, q = rc.spread_data()
    yield "spread-f32", q, x, rc.score_ids(len(x), len(q), 9)
    for storage in ("bf16", "fp8_e4m3", "fp8_e4m3_docs"):
        _, xs = rc.rows_data(storage, 100, 129)
        qs = rc.lc.stored_queries(rc.rows_data("f32", 100, 5, seed=2)[0], storage)
        yield storage, qs, xs, rc.score_ids(129, 5, 37)


@pytest.mark.parametrize("mutant", ["pairwise", "l2_as_ip"])
def test_a_wrong_score_kernel_fails_a_case(mutant):
    failed = []
    for name, q, x, ids in _score_cases():
        phi = float(rc.orc.sumsq_canonical(x).max())
        for metric in (0, 1):
            exp = rc.model_scores(q, x, ids, metric, phi)
            assert np.array_equal(rc.kernel_scores(q, x, ids, metric, phi).view(np.uint32), exp.view(np.uint32))
            assert np.all(np.isinf(exp[ids < 0])) and np.all((exp[ids < 0] > 0) == (metric == 1))
            if not np.array_equal(rc.kernel_scores(q, x, ids, metric, phi, mutant).view(np.uint32), exp.view(np.uint32)):
                failed.append((name, metric))
    assert failed, mutant
    if mutant == "pairwise":
        assert ("spread-f32", 0) in failed                                         # the order of the sum is visible there
    else:
        assert all(m == 1 for _, m in failed) and len(failed) == 4                 # every L2 case, no inner-product case


def test_model_scores_is_the_oracle_search():
    from oracle import mips_oracle as orc

    _, x = rc.rows_data("bf16", 100, 500)
    q = rc.lc.stored_queries(rc.rows_data("f32", 100, 7, seed=2)[0], "bf16")
    for metric in (0, 1):
        D, I = orc.search_exact(q, x, 12, metric=metric)
        got = rc.model_scores(q, x, I, metric, float(orc.sumsq_canonical(x).max()))
        assert np.array_equal(got.view(np.uint32), D.view(np.uint32))


# ------------------------------------------------------------------ 3. the shim's L2 column
def test_l2_column_formula():
    from oracle import mips_oracle as orc

    x = rc.rows_data("f32", 33, 50)[0]
    phi = float(orc.sumsq_canonical(x).max())
    col = ram.faiss_shim.l2_augmentation_column(x, phi)
    assert col.dtype == np.float32 and np.array_equal(col, rc.l2_column(x, phi))
    assert col[int(np.argmax(orc.sumsq_canonical(x)))] == 0.0                      # the longest row sits on the sphere already
    aug = orc.augment_xb(x, phi)                                                   # the reference's augmentation of the same rows
    assert np.allclose(col, aug[:, -1], rtol=1e-5, atol=1e-3 * np.sqrt(phi))
    assert np.array_equal(ram.faiss_shim.l2_augmentation_column(x, phi * 0.5) == 0, orc.sumsq_canonical(x) >= phi * 0.5)
    nan_row = np.full((1, 33), np.nan, np.float32)
    assert np.isnan(ram.faiss_shim.l2_augmentation_column(nan_row, phi)).all()     # "no row" stays NaN in the column too


def test_shim_refuses_an_empty_index_without_a_gpu():
    ix = ram.faiss_shim.IndexFlat(8, ram.faiss_shim.METRIC_INNER_PRODUCT)
    with pytest.raises(IndexError):
        ix.reconstruct(0)
    assert ix.reconstruct_n().shape == (0, 8) and ix.reconstruct_batch(np.zeros(0, np.int64)).shape == (0, 8)
    assert ix.reconstruct_batch(np.zeros((2, 0), np.int64)).shape == (2, 0, 8)
    with pytest.raises(IndexError):
        ix.reconstruct_batch(np.array([0]))


# ------------------------------------------------------------------ 4. sharded plumbing on gloo, injected local step
def _gloo_worker(rank, world, port, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x = rc.planted_f32(129, 20)                                # -0.0, denormals and NaN payloads cross the all-reduce
        counts = [100, 29][:world] if world == 2 else [60, 0, 69]  # uneven shards, as remove_ids_global leaves them
        lo, hi, n = ram.shard_offsets(counts, rank)
        calls = []

        def local_reconstruct(ids, off):
            assert off == lo and isinstance(ids, np.ndarray) and ids.dtype == np.int64 and ids.ndim == 1
            calls.append(len(ids))
            return rc.model_reconstruct(x[lo:hi], ids, off, zero_missing=True)

        ix = ram.ShardedMipsIndex(20, local_reconstruct=local_reconstruct)
        assert ix.local is None and (ix.rank, ix.world) == (rank, world)
        ix.lo, ix.hi, ix.ntotal_global, ix._even = lo, hi, n, False
        ids = np.concatenate([np.arange(n)[::-1], [-1, n, (1 << 32) + 3, rc.INT64_MIN, 3, 3, 128]]).astype(np.int64).reshape(8, 17)
        got = ix.reconstruct_batch(ids)
        exp = rc.model_reconstruct(x, ids)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (8, 17, 20)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
        assert (got.view(np.uint32) == 0x80000000).sum() == (exp.view(np.uint32) == 0x80000000).sum() > 20
        assert calls == [8 * 17]
        every = [None] * world
        dist.all_gather_object(every, got.tobytes())
        assert all(e == every[0] for e in every)
        # a float sum would not do: it loses the sign of -0.0
        import torch
        assert torch.equal(torch.tensor([-0.0]) + torch.tensor([0.0]), torch.tensor([0.0])) and not torch.signbit(torch.tensor([-0.0]) + torch.tensor([0.0])).any()
        assert ix.reconstruct_batch(np.zeros((0, 3), np.int64)).shape == (0, 3, 20)
        ret[rank] = True
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_reconstruct_on_gloo_with_an_injected_local_step(world):
    import torch.multiprocessing as mp

    port = 28700 + (os.getpid() % 2000) + 7 * world
    ret = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, port, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}
