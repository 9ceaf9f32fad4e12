"""GPU (-m gpu): the resident dataset (garmentnets_amd/io/resident.py, csrc/resident.hip) against the host dataset it replaces.

The yardstick is GarmentInputDataset with static_epoch_seed=True (itself pinned to the reference by tests/golden/ref_dataset.npz): for every case
`ResidentDataset.batch(chunk)` is compared, field by field and with no field left out, with `collate([dataset[k] for k in chunk]).to(device)`.

Rule A, bit equality (torch.equal): every field no fp32 rotation touches -- all of them without augmentation; with it everything but the rotated
fields below; with pc_noise_std > 0 also `pos` (its rotation is an fp64 product rounded once).

Rule B, the rotated fp32 fields (`pos` without noise, `sim_grip_point`, `gt_sim_points`; in task space the two pivoted query fields instead of
`gt_sim_points`): numpy's matmul goes through BLAS and may fuse, so bit equality is not owed.  Two correctly ordered 3-term fp32 dot products differ by at
most 2 gamma_3 sum|x_i||r_i| <= 6 * 2**-24 * (|x| + |y| + |z|) with |R| <= 1; the bound is applied per element with the UN-ROTATED host row (the same
seeded dataset with enable_augumentation=False) on the right-hand side.  The pivoted fields are fl(dot(q - pivot) + pivot): the row entering the dot
product is q - pivot (computed identically on both sides), and the final addition rounds once on either side, so their bound is
6 * 2**-24 * |q - pivot|_1 + 2 * 2**-24 * max(|ours|, |host|): the dot products' bound plus one rounding of relative size 2**-24 per side.  Derived,
not measured.  Measured on an MI355X host: the plain fields at most 3.0e-8 against bounds of 2.7e-7 .. 5.5e-7, the pivoted ones 1.2e-7 against 8.6e-7.

End to end (`--static_epoch_seed --no_augmentation`, two epochs, --num_batches 2 on a 20-sample store): the host path run twice is bit-identical, and so
is the --resident run against it -- train_* and val_* values, every tensor of last.ckpt and the optimiser state -- for train_pipeline and for train.

The stores are awkward on purpose (write_awkward_store): clouds of different stored lengths, a view table with an empty view, a one-face mesh, repeated
and zero-area faces, volume size 5 in one store and 12 in the other.
"""
import csv

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import train as T  # noqa: E402
from garmentnets_amd import train_pipeline as TP  # noqa: E402
from garmentnets_amd.io import zarr_store  # noqa: E402
from garmentnets_amd.io.dataset import TASK_SPACE_VOLUME_GROUP, GarmentInputDataset  # noqa: E402
from garmentnets_amd.io.resident import ResidentDataset  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
VIEWS = [[37, 0, 601, 130], [200, 300, 100, 300], [192, 192, 192, 192], [400, 150, 250, 200], [130, 420, 120, 180]]
VERTS = [40, 3, 25, 60, 33]
GROUPS = ("nocs_winding_number_field", "nocs_occupancy_grid", "nocs_signed_distance_field", TASK_SPACE_VOLUME_GROUP)
ORDER = [4, 0, 1, 2, 3]                                            # resident slot != dataset index


def _mesh_faces(rng, i, nverts):
    if i == 1:
        return np.array([[0, 1, 2]], dtype=np.int32)                 # the one-face mesh
    f = rng.integers(0, nverts, (30 + 20 * i, 3)).astype(np.int32)
    f[3:9] = f[2]                                                    # repeated faces
    f[12:17, 2] = f[12:17, 0]                                        # zero-area faces
    return f


def write_awkward_store(path, volume_size, seed=0):
    rng = np.random.default_rng(seed)
    root = zarr_store.open_group(path)
    root.require_group("summary").array("cloth_aabb_union", np.array([[-0.4, -0.4, -0.9], [0.4, 0.4, 0.05]], dtype=np.float32))
    box = lambda n: (rng.random((n, 3)) * [0.7, 0.7, 0.9] + [-0.35, -0.35, -0.88]).astype(np.float32)
    for i, views in enumerate(VIEWS):
        sg = root.require_group("samples").require_group(f"{i:05d}_Dress_{i:06d}_0")
        sg.put_attrs({"scale": 1.0 + 0.1 * i, "sample_id": f"{i:05d}_Dress", "garment_name": "Dress", "grip_vertex_idx": (7 * i + 2) % VERTS[i]})
        n = sum(views)
        pc, mesh, mc = sg.require_group("point_cloud"), sg.require_group("mesh"), sg.require_group("marching_cube_mesh")
        pc.array("point", box(n), chunks=(500, 3), compressor=("zlib", 1))
        pc.array("nocs", rng.random((n, 3)).astype(np.float32))
        pc.array("rgb", rng.integers(0, 256, (n, 3)).astype(np.uint8))
        pc.array("sizes", np.array(views, dtype=np.int64))
        mesh.array("cloth_verts", box(VERTS[i]))
        mesh.array("cloth_nocs_verts", rng.random((VERTS[i], 3)).astype(np.float32))
        mesh.array("cloth_faces_tri", _mesh_faces(rng, i, VERTS[i]))
        mv = 20 + 9 * i
        mc.array("marching_cube_verts", rng.random((mv, 3)).astype(np.float32), chunks=(16, 3), compressor=("zlib", 1))
        mc.array("marching_cube_faces", _mesh_faces(rng, (i + 1) % 5, mv))
        mc.array("is_vertex_on_surface", rng.random(mv) > 0.4)
        vol = sg.require_group("volume")
        for grp in GROUPS:
            v = rng.random((volume_size,) * 3).astype(np.float32)
            if grp == "nocs_signed_distance_field":
                v = (v - 0.5) * 0.3                                  # beyond tsdf_clip_value = 0.05 on both sides
            vol.require_group(grp).array(str(volume_size), v, compressor=("zlib", 1))


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    root = tmp_path_factory.mktemp("resident")
    out = {}
    for size in (5, 12):
        out[size] = str(root / f"v{size}.zarr")
        write_awkward_store(out[size], size, seed=size)
    return out


BASE = dict(num_pc_sample=333, num_views=4, num_volume_sample=257, num_surface_sample=131, static_epoch_seed=True, enable_augumentation=False,
            random_rot_range=(-180, 180))
# name -> (volume size, dataset keywords over BASE, chunk)
CASES = {
    "plain": (5, {}, ORDER),
    "whole_pool": (5, dict(num_pc_sample=768), [0, 2]),                                    # P == the stored cloud of both garments
    "views_below_stored": (5, dict(num_views=3, num_pc_sample=100, enable_augumentation=True), [1, 0, 3]),
    "one_garment": (5, dict(enable_augumentation=True), [3]),
    "repeated_index": (5, {}, [2, 2, 0, 2]),
    "near_surface": (5, dict(surface_sample_ratio=0.5, surface_sample_std=0.5, enable_augumentation=True), ORDER),
    "mc_surface": (5, dict(num_mc_surface_sample=50, enable_augumentation=True), [1, 4, 0]),
    "occupancy": (5, dict(volume_group="nocs_occupancy_grid", surface_sample_ratio=0.5, surface_sample_std=0.5), [0, 1, 2]),
    "tsdf_abs": (5, dict(volume_group="nocs_signed_distance_field", tsdf_clip_value=0.05, volume_absolute_value=True), [2, 3, 4]),
    "task_space": (5, dict(volume_group=TASK_SPACE_VOLUME_GROUP, surface_sample_ratio=0.25, surface_sample_std=0.5, enable_augumentation=True), ORDER),
    "task_space_no_aug": (5, dict(volume_group=TASK_SPACE_VOLUME_GROUP, surface_sample_ratio=0.25), [1, 3]),
    "noise": (5, dict(pc_noise_std=0.01), [0, 1, 4]),
    "noise_aug": (5, dict(pc_noise_std=0.01, enable_augumentation=True), [0, 1, 4]),
    "volume12": (12, dict(surface_sample_ratio=0.5, surface_sample_std=0.5, enable_augumentation=True), ORDER),
    "volume12_no_targets": (12, dict(num_volume_sample=0, num_surface_sample=0, enable_augumentation=True), [4, 1]),
}


def _dataset(stores, size, **kw):
    return GarmentInputDataset(stores[size], volume_size=size, **{**BASE, **kw})


def _host(ds, chunk):
    return GarmentInputDataset.collate([ds[k] for k in chunk])


def rotated_fields(ds):
    """field -> pivoted?  for the fields an fp32 rotation touches (Rule B)"""
    if not ds.enable_augumentation:
        return {}
    out = {"sim_grip_point": False}
    if ds.pc_noise_std == 0:
        out["pos"] = False
    if ds.volume_task_space:
        if ds.num_volume_sample > 0:
            out["volume_query_points"] = True
        if ds.num_surface_sample > 0:
            out["surf_query_points"] = True
    elif ds.num_surface_sample > 0:
        out["gt_sim_points"] = False
    return out


def compare(got, host, plain_host, ds, tag):
    """every field of the host batch against the resident one: Rule B for rotated_fields(ds) (plain_host: the same batch un-rotated), Rule A for the rest"""
    assert set(got.keys) == set(host.keys), (tag, sorted(set(got.keys) ^ set(host.keys)))
    assert got.sizes == host.sizes and got.num_graphs == host.num_graphs
    rule_b = rotated_fields(ds)
    worst = {}
    for k in host.keys:
        g, h = getattr(got, k), getattr(host, k)
        assert g.device.type == "cuda" and g.shape == h.shape and g.dtype == h.dtype, (tag, k, g.shape, h.shape, g.dtype, h.dtype)
        g = g.cpu()
        if k not in rule_b:
            assert torch.equal(g, h), (tag, k, "Rule A", float((g.double() - h.double()).abs().max()))
            continue
        plain = getattr(plain_host, k).double()
        if rule_b[k]:
            row = plain - torch.tensor([0.5, 0.5, 0.0], dtype=torch.float64)
            bound = 6 * U * row.abs().sum(-1, keepdim=True) + 2 * U * torch.maximum(g.abs(), h.abs()).double()
        else:
            bound = (6 * U * plain.abs().sum(-1, keepdim=True)).expand_as(plain)
        err = (g.double() - h.double()).abs()
        worst[k] = (float(err.max()), float(bound.max()))
        assert bool((err <= bound).all()), (tag, k, "Rule B", worst[k])
    print(f"[resident] {tag}: Rule B max error / max bound {worst}")


@pytest.fixture(scope="module")
def residents(stores):
    """case -> (dataset, resident dataset, host batch, un-rotated host batch), built once"""
    cache = {}

    def get(name):
        if name not in cache:
            size, kw, chunk = CASES[name]
            ds = _dataset(stores, size, **kw)
            host = _host(ds, chunk)
            plain = _host(_dataset(stores, size, **{**kw, "enable_augumentation": False}), chunk) if ds.enable_augumentation else host
            cache[name] = (ds, ResidentDataset(ds, ORDER, DEV), host, plain)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_batch_matches_the_host_dataset(residents, name):
    ds, res, host, plain = residents(name)
    chunk = CASES[name][2]
    got = res.batch(chunk)
    compare(got, host, plain, ds, name)
    again = res.batch(chunk)                                            # seeded: two calls, the same bits
    for k in got.keys:
        assert torch.equal(getattr(got, k), getattr(again, k)), (name, k)
    assert got.dataset_idx.tolist() == chunk
    if not ds.enable_augumentation:
        assert torch.equal(got.input_aug_rot_mat.cpu(), torch.eye(3).expand(len(chunk), 3, 3))


def test_many_batches_reuse_the_draw_buffers(residents, stores):
    """more batches than pinned draw buffers, of changing size, none read back in between: every one still the host's"""
    ds, res, _, _ = residents("near_surface")
    plain_ds = _dataset(stores, 5, **{**CASES["near_surface"][1], "enable_augumentation": False})
    chunks = [[0], [1, 2, 3], [4, 0], [2], [3, 3, 1, 0, 4], [1]]
    got = [res.batch(c) for c in chunks]
    for c, g in zip(chunks, got):
        compare(g, _host(ds, c), _host(plain_ds, c), ds, f"ring {c}")


def test_unseeded_batches_differ_and_stay_inside_the_sample(stores):
    ds = _dataset(stores, 5, static_epoch_seed=False, surface_sample_ratio=0.5, surface_sample_std=0.5)
    res = ResidentDataset(ds, ORDER, DEV)
    chunk = [0, 1, 1, 3]
    a, b = res.batch(chunk), res.batch(chunk)
    assert not torch.equal(a.pos, b.pos) and not torch.equal(a.volume_query_points, b.volume_query_points)
    assert not torch.equal(a.surf_query_points, b.surf_query_points)
    P = ds.num_pc_sample
    for g, k in enumerate(chunk):
        raw = ds.samples_group[ds.keys[k]]["point_cloud"]
        stored = {r.tobytes() for r in np.concatenate([raw["point"].astype(np.float32), raw["nocs"].astype(np.float32)], axis=1)}
        rows = torch.cat([a.pos[g * P:(g + 1) * P], a.y[g * P:(g + 1) * P]], dim=1).cpu().numpy()
        assert all(r.tobytes() in stored for r in rows), k                              # every row a stored row of ITS garment
        assert len({r.tobytes() for r in rows}) == P                                     # drawn without replacement
    for t in (a.volume_query_points, a.surf_query_points, a.gt_volume_value):
        assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    assert bool((a.volume_query_points == 0).any()) and bool((a.volume_query_points == 1).any())      # std 0.5: many queries clipped
    assert a.dataset_idx.tolist() == chunk


def test_budget_refusal_names_both_figures_and_allocates_nothing(stores):
    ds = _dataset(stores, 12)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(ValueError) as e:
        ResidentDataset(ds, ORDER, DEV, max_bytes=1)
    need = ResidentDataset(ds, ORDER, DEV).nbytes
    assert str(need) in str(e.value) and " 1 bytes" in str(e.value)
    assert torch.cuda.memory_allocated(DEV) == before
    assert need >= 5 * 12 ** 3 * 4 and ResidentDataset(ds, ORDER, DEV, max_bytes=need).nbytes == need


def test_nbytes_is_the_sum_of_the_resident_tensors(stores):
    res = ResidentDataset(_dataset(stores, 5, num_mc_surface_sample=10, surface_sample_ratio=0.5), ORDER, DEV)
    assert res.nbytes == sum(t.numel() * t.element_size() for t in res.arrays.values())
    assert res.load_seconds > 0 and len(res) == 5


def test_an_index_that_is_not_resident_raises_keyerror(stores):
    res = ResidentDataset(_dataset(stores, 5), [0, 1, 2], DEV)
    with pytest.raises(KeyError):
        res.batch([1, 4])
    assert res.batch([2, 0]).dataset_idx.tolist() == [2, 0]


# ------------------------------------------------------------------------------------------------ end to end
def _equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_equal(v, b[k]) for k, v in a.items())
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b


def _same_run(a, b, out_a, out_b, prefix_train, tag):
    rows_a = [{k: v for k, v in r.items() if k.startswith(prefix_train)} for r in a["train_rows"]]
    rows_b = [{k: v for k, v in r.items() if k.startswith(prefix_train)} for r in b["train_rows"]]
    assert rows_a == rows_b and len(rows_a) == 4, (tag, rows_a, rows_b)
    val_a = [{k: v for k, v in e.items() if k.startswith("val_")} for e in a["val_epochs"]]
    val_b = [{k: v for k, v in e.items() if k.startswith("val_")} for e in b["val_epochs"]]
    assert val_a == val_b and len(val_a) == 2, (tag, val_a, val_b)
    ck_a = torch.load(str(out_a / "checkpoints" / "last.ckpt"), map_location="cpu", weights_only=False)
    ck_b = torch.load(str(out_b / "checkpoints" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert set(ck_a["state_dict"]) == set(ck_b["state_dict"])
    differ = [k for k, v in ck_a["state_dict"].items() if not torch.equal(v, ck_b["state_dict"][k])]
    assert not differ, (tag, differ)
    assert _equal(ck_a["optimizer_states"][0]["state"], ck_b["optimizer_states"][0]["state"]), (tag, "optimizer state")


@pytest.fixture(scope="module")
def train_store(tmp_path_factory):
    from test_validate_host import VOLUME_SIZE, write_validation_store
    store = tmp_path_factory.mktemp("resident_train") / "ds.zarr"
    write_validation_store(str(store), 20)
    return ["--zarr_in", str(store), "--volume_size", str(VOLUME_SIZE), "--epochs", "2", "--batch_size", "2", "--num_pc_sample", "400", "--num_batches", "2",
            "--static_epoch_seed", "--no_augmentation"]


def test_train_pipeline_main_resident_run_is_the_host_run(train_store, tmp_path):
    common = train_store + ["--num_volume_sample", "96", "--num_surface_sample", "80", "--grid", "8"]
    runs = {}
    for name, extra in (("host", []), ("host2", []), ("resident", ["--resident"])):
        runs[name] = TP.main(common + ["--output_dir", str(tmp_path / name)] + extra)
    _same_run(runs["host"], runs["host2"], tmp_path / "host", tmp_path / "host2", "train_", "pipeline: host against host")
    _same_run(runs["host"], runs["resident"], tmp_path / "host", tmp_path / "resident", "train_", "pipeline: resident against host")
    rows = list(csv.DictReader(open(tmp_path / "resident" / "train_metrics.csv")))
    assert len(rows) == 4 and all(r["resident"] == "True" and float(r["data_seconds"]) > 0 for r in rows)
    assert "resident" not in list(csv.DictReader(open(tmp_path / "host" / "train_metrics.csv")))[0]


def test_train_main_resident_run_is_the_host_run(train_store, tmp_path):
    common = train_store + ["--model", "pointnet2"]
    host = T.main(common + ["--output_dir", str(tmp_path / "host")])
    res = T.main(common + ["--output_dir", str(tmp_path / "resident"), "--resident", "--resident_gib", "0.5"])
    _same_run(host, res, tmp_path / "host", tmp_path / "resident", "train_", "first stage: resident against host")


def test_shuffled_resident_epochs_visit_the_permutation(train_store, tmp_path):
    common = train_store + ["--num_volume_sample", "96", "--num_surface_sample", "80", "--grid", "8", "--resident", "--shuffle", "--seed", "3"]
    seen = []
    real = ResidentDataset.batch

    def spy(self, chunk):
        seen.append(list(chunk))
        return real(self, chunk)
    ResidentDataset.batch = spy
    try:
        out = TP.main(common + ["--output_dir", str(tmp_path / "s")])
    finally:
        ResidentDataset.batch = real
    from garmentnets_amd import train_loop as L
    assert len(out["train_rows"]) == 4
    train_idx = GarmentInputDataset(train_store[1], volume_size=int(train_store[3])).subset_indices("train")
    want = [L.epoch_order(train_idx, True, 3, e)[:4].tolist() for e in range(2)]
    train_chunks = [c for c in seen if set(c) <= set(train_idx.tolist())]
    assert [sum(train_chunks[2 * e:2 * e + 2], []) for e in range(2)] == want and want[0] != want[1]
