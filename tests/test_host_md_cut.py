"""CPU: the condition tests/test_gpu_md_cut.py puts on its own inputs, decided from the restatement of tests/md_cut_refs.py alone: every
restated state under the cutoff is finite, and at most one in ten (item, step count) pairs is not steady in the sense of
tests/test_gpu_md.py (_gate_state) -- the cap tests/test_host_md_steps.py uses -- so that the gate is calibrated by the unturned fp32
run on nearly all items."""
import torch

import md_cut_refs as mc
import md_steps_refs as ms
import nb_cut_refs as nc


def test_the_cutoffs_of_the_dynamics_cases_are_placed_in_a_gap():
    for name in mc.CASES + ["nve"]:
        b = ms.nve_batch() if name == "nve" else ms.case(name)
        rc, half = nc.place_cutoff(b.params, b.xyz.numpy(), mc.NOMINAL)
        cut = mc.cutoff(name)
        assert cut.distance == rc and abs(rc - mc.NOMINAL) <= nc.WINDOW + 1e-6 and half >= 1e-4, (name, rc, half)
        assert abs(cut.switch_distance - 0.8 * rc) < 1e-12 and cut.rf_dielectric == 78.3


def test_the_restated_force_is_the_cut_one_only_inside_the_context():
    b = ms.case("s65_C3")
    import relax_refs as rr
    plain = rr.forces(b, b.xyz, torch.float64)["E"]
    with mc.cut_force(nc.Cutoff(4.0)):
        cut = rr.forces(b, b.xyz, torch.float64)["E"]
    assert not torch.equal(plain, cut) and torch.equal(plain, rr.forces(b, b.xyz, torch.float64)["E"])


def test_the_inputs_of_the_gpu_tests_are_finite_and_mostly_steady():
    for name in mc.CASES:
        for real in mc.verlet32(name):
            for k in mc.TRAJ_STEPS:
                for state in real[k]:
                    assert bool(torch.isfinite(state[0]).all()) and bool(torch.isfinite(state[1]).all()), (name, k)
    n = mc.steady_counts()
    print(f"not steady under the cutoff: x {n['x'][0]} of {n['x'][1]}, v {n['v'][0]} of {n['v'][1]} (item, step count) pairs")
    assert 10 * n["x"][0] <= n["x"][1] and 10 * n["v"][0] <= n["v"][1], n
