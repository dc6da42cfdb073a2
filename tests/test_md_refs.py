"""CPU: the host side of the dynamics (the library's Philox4x32-10 against the numpy restatement and Random123's known answers, the
option checks, the molecule keys) and the conditions the GPU tests of tests/test_gpu_md.py put on their own inputs, established for the
float64 restatement of tests/md_refs.py alone."""
import numpy as np
import pytest
import torch

import md_refs as md
from grappa_amd import _lib
from grappa_amd.dynamics import MD_DEFAULTS, md_options, mol_keys


def test_library_philox_is_the_restatement_and_random123():
    for ctr, (k0, k1), want in md.KAT:
        assert _lib.md_philox(k0 | (k1 << 32), *ctr) == want
        assert tuple(int(w) for w in md.philox(np.uint64(k0 | (k1 << 32)), *ctr)) == want
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 2 ** 64, size=3000, dtype=np.uint64)
    ctr = rng.integers(0, 2 ** 32, size=(3000, 4), dtype=np.uint64)
    # the edges: zero and all-ones in every position, small counters as the kernel forms them
    keys[:4] = [0, 2 ** 64 - 1, 0, 2 ** 64 - 1]
    ctr[:4] = [[0, 0, 0, 0], [2 ** 32 - 1] * 4, [2 ** 32 - 1] * 4, [0, 0, 0, 0]]
    ctr[4:300] = rng.integers(0, 4, size=(296, 4))
    want = md.philox(keys, ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3])
    for k in range(3000):
        assert _lib.md_philox(int(keys[k]), *(int(c) for c in ctr[k])) == tuple(int(w) for w in want[k]), k


def test_every_counter_word_and_key_half_changes_the_output():
    base = dict(key=0x0123456789ABCDEF, c=[5, 6, 7, 0])
    ref = _lib.md_philox(base["key"], *base["c"])
    seen = {ref}
    for pos in range(4):
        c = list(base["c"])
        c[pos] += 1
        seen.add(_lib.md_philox(base["key"], *c))
    seen.add(_lib.md_philox(base["key"] ^ 1, *base["c"]))
    seen.add(_lib.md_philox(base["key"] ^ (1 << 32), *base["c"]))
    assert len(seen) == 7
    assert len({w for out in seen for w in out}) == 28          # no word repeats either


def test_box_muller_never_sees_zero_and_is_standard_normal():
    """the extreme words give finite deviates, and 98,304 values of the restatement pass the bounds the GPU test puts on the kernel"""
    w = np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint64) >> np.uint64(8)
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -24
    assert u.min() > 0 and u.max() < 1 and np.sqrt(-2 * np.log(u)).max() < 5.9
    z = md.noise_ref([512], md.keys("max"), 64, 3, 0).numpy().reshape(-1)
    n = z.shape[0]
    assert n == 98304 and abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert np.abs(z).max() < 5.9


def test_noise_depends_on_purpose_step_key_atom_and_conformation():
    k = md.keys("mixed")
    base = md.noise_ref([3, 2], k[:2], 2, 4, 0)
    assert not torch.equal(base, md.noise_ref([3, 2], k[:2], 2, 4, 1)) and not torch.equal(base, md.noise_ref([3, 2], k[:2], 2, 5, 0))
    assert not torch.equal(base, md.noise_ref([3, 2], k[1:3], 2, 4, 0))
    assert len({float(v) for v in base.reshape(-1)}) == base.numel()
    # a molecule's noise is its own: the same key gives the same rows wherever the molecule stands in the batch
    assert torch.equal(md.noise_ref([2, 3], k[[1, 0]], 2, 4, 0)[2:], base[:3])


def test_md_options():
    o = md_options()
    assert o == {**MD_DEFAULTS, "init_temperature": MD_DEFAULTS["temperature"]} and o["dt"] == 0.001 and o["friction"] == 1.0
    assert md_options(temperature=500.0)["init_temperature"] == 500.0 and md_options(init_temperature=0.0)["init_temperature"] == 0.0
    assert md_options(n_steps=7.0)["n_steps"] == 7 and isinstance(md_options(n_steps=7.0)["n_steps"], int)
    with pytest.raises(TypeError, match="unknown"):
        md_options(timestep=0.001)
    for bad in ({"dt": 0.0}, {"dt": -1.0}, {"dt": float("nan")}, {"dt": float("inf")}, {"temperature": -1.0}, {"temperature": float("nan")},
                {"friction": -0.1}, {"friction": float("inf")}, {"init_temperature": -1.0}, {"n_steps": -1}, {"n_steps": 1.5},
                {"save_every": -1}, {"save_every": True}, {"dt": "fast"}):
        with pytest.raises(ValueError):
            md_options(**bad)


def test_mol_keys_are_distinct_and_reproducible():
    a = mol_keys(11, 1000)
    assert a.dtype == np.uint64 and len(set(a.tolist())) == 1000
    assert np.array_equal(a, mol_keys(11, 1000)) and np.array_equal(a[:10], mol_keys(11, 10))
    assert not set(a.tolist()) & set(mol_keys(12, 1000).tolist())
    # splitmix64's first outputs for seed 0 (Vigna's reference implementation)
    assert mol_keys(0, 3).tolist() == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError):
            mol_keys(bad, 2)


def test_restatement_conserves_energy_and_keeps_frozen_atoms():
    """velocity Verlet on the 9-atom molecule: the total energy of the float64 restatement stays within the O(dt^2) band over 80
    steps and a quarter of the step shrinks the band about sixteenfold; a mass-0 atom does not move"""
    b, m = md.case("n9_C3"), md.masses("n9_C3").copy()
    v = md.thermal_velocities("n9_C3")
    band = []
    for dt, n in ((0.0005, 80), (0.000125, 320)):
        r = md.baoab_ref(b, m, velocities=v, dt=dt, n_steps=n, save_every=n // 20)
        e = r["frame_epot"] + r["frame_ekin"]
        band.append(float((e - e[0]).abs().max()))
    assert band[1] < band[0] / 8, band
    m[4] = 0.0
    r = md.baoab_ref(b, m, velocities=v, dt=0.0005, n_steps=20)
    assert torch.equal(r["xyz"][4], b.xyz[4].double()) and not r["vel"][4].any() and bool((r["xyz"][3] != b.xyz[3].double()).all())


def test_equipartition_of_the_float64_restatement():
    """the condition on the input of the GPU equipartition test: |mean_f64 - 300| <= 5 se + a 300 with a = twice BAOAB's harmonic bias
    of the stiffest bond, and a <= 0.03 at the step the test uses"""
    a = md.harmonic_bias("n9_C64", md.NVT["dt"])
    assert a <= 0.03, a
    r = md.nvt()
    assert bool((r["status"] == 0).all()) and bool(r["written"].all())
    mean, se = md.replica_temperature(r["frame_ekin"], 9)
    print(f"float64 restatement: kinetic temperature {mean:.2f} +- {se:.2f} K over 64 replicas, a = {a:.4f}")
    assert abs(mean - md.NVT["temperature"]) <= 5 * se + a * md.NVT["temperature"], (mean, se, a)
