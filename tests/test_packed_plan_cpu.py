"""Host side of the packed plan (gcdm_plan_batches / gcdm_set_batch_seeds, mol_gen_sample_packed, sample_and_analyze(packed_batches=)): what can be
checked without a GPU -- the header and the binding agree on the two new exports, the header still compiles and links from plain C, and the Python
drivers refuse inconsistent arguments before any device call (this suite runs where there is no device: a device call would raise something else)."""
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gcdm_hip.h")
NEW = ("gcdm_plan_batches", "gcdm_set_batch_seeds")


def test_header_and_binding_declare_the_new_exports():
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(gcdm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in native.EXPORTS, name
    assert re.search(r"int\s+gcdm_plan_batches\(gcdm_handle\*\s*h,\s*int32_t\s+num_batches,\s*const int32_t\*\s*molecules_per_batch,\s*const int32_t\*\s*num_nodes\);", hdr)
    assert re.search(r"int\s+gcdm_set_batch_seeds\(gcdm_handle\*\s*h,\s*int32_t\s+num_batches,\s*const uint64_t\*\s*host_seeds\);", hdr)
    assert "IGNORED" in hdr[hdr.index("Packed plan"):hdr.index("int gcdm_plan_batches")]          # the scalar seed under a packed plan
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integ for name in NEW)


def test_header_compiles_and_links_from_plain_c(tmp_path):
    """The two new entry points through the header from C99: their null-handle error paths need no GPU."""
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("library not built")
    gcc = shutil.which("gcc")
    assert gcc is not None, "no gcc"
    src = tmp_path / "packed.c"
    src.write_text("""
#include "gcdm_hip.h"
#include <stdio.h>
int main(void) {
    const int32_t per[2] = {2, 1}, nn[3] = {4, 5, 3};
    const uint64_t seeds[2] = {1234u, 1235u};
    int (*plan)(gcdm_handle*, int32_t, const int32_t*, const int32_t*) = gcdm_plan_batches;
    int (*seed)(gcdm_handle*, int32_t, const uint64_t*) = gcdm_set_batch_seeds;
    if (plan(NULL, 2, per, nn) == 0) return 1;
    if (seed(NULL, 2, seeds) == 0) return 2;
    if (gcdm_get_option(NULL, "num_batches") != -1) return 3;
    puts("ok");
    return 0;
}
""")
    exe = tmp_path / "packed"
    libdir = os.path.dirname(native.LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe),
                        "-L" + libdir, "-lgcdm_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)


@pytest.fixture(scope="module")
def model():
    return pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9"))


def test_packed_sampler_rejects_inconsistent_lists_before_any_device_call(model):
    ddpm = model.ddpm
    two = [torch.tensor([4, 5]), torch.tensor([3])]
    with pytest.raises(ValueError, match="seeds"):
        ddpm.mol_gen_sample_packed(two, "cuda", num_timesteps=2, seeds=[1])
    with pytest.raises(ValueError, match="contexts"):
        ddpm.mol_gen_sample_packed(two, "cuda", num_timesteps=2, contexts=[None, None, None])
    with pytest.raises(ValueError, match="empty"):
        ddpm.mol_gen_sample_packed([torch.tensor([4, 5]), torch.tensor([], dtype=torch.long)], "cuda", num_timesteps=2)
    with pytest.raises(ValueError, match="empty"):
        ddpm.mol_gen_sample_packed([], "cuda", num_timesteps=2)


def test_packed_sampler_refuses_a_self_conditioned_model(model):
    dyn = model.ddpm.dynamics_network
    had = getattr(dyn, "self_condition", False)
    dyn.self_condition = True
    try:
        with pytest.raises(NotImplementedError, match="self-conditioned"):
            model.ddpm.mol_gen_sample_packed([torch.tensor([4, 5])], "cuda", num_timesteps=2)
    finally:
        dyn.self_condition = had


def test_evaluation_driver_rejects_packed_together_with_concurrent(model):
    with pytest.raises(ValueError, match="exclude"):
        model.sample_and_analyze(num_samples=4, batch_size=2, num_timesteps=2, concurrent_batches=2, packed_batches=2)
    with pytest.raises(ValueError, match="packed_batches"):
        model.sample_and_analyze(num_samples=4, batch_size=2, num_timesteps=2, packed_batches=0)
