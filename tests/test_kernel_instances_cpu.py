"""Which template instances of the kernels the built library holds -- read from the library file, no GPU, nothing loaded onto a
device.

The exact mode has ONE operand type (ExactEl = F16, csrc/bmu_exact.hpp) and its host side is no template on it, so the library
must hold no bfloat16 twin of an exact-mode kernel: such a twin cannot be launched, and it cost a quarter of the library and of
every build.  The kernels' descriptors (<mangled name>.kd) are symbols of the code object inside the library; `4Bf16` / `3F16` in
a mangled name are the operand type's tag.  Only names are read here, never a kernel's instructions."""
import collections
import re

import pytest

from xpysom_dask_amd import _lib

# the scan kernels' flags <.., EL, GM, TL, T2> (bmu_bf16_k16_kernel) and <.., EL, GM, TL, PLAN> (bmu_bf16_wide_kernel)
PLAIN = "Lb0ELb0ELb0E"
K16_VARIANTS = {PLAIN, "Lb1ELb0ELb0E", "Lb1ELb1ELb0E", "Lb0ELb1ELb0E", "Lb1ELb0ELb1E"}      # plain, GM, GM+TL, TL, GM+T2
WIDE_VARIANTS = {PLAIN, "Lb1ELb0ELb0E", "Lb1ELb1ELb0E", "Lb0ELb1ELb0E", "Lb0ELb0ELb1E"}     # plain, GM, GM+TL, TL, PLAN
# every kernel with a bfloat16 instance: precision 'bf16' and the MFMA probe
BF16_KERNELS = {"bmu_bf16_k16_kernel", "bmu_bf16_wide_kernel", "bmu_bf16_tiled_kernel", "prep_w_bf16_k16_kernel",
                "merge_prep_k16_kernel", "prep_w_bf16_wide_kernel", "merge_prep_wide_kernel", "prep_tiles_bf16_kernel",
                "prep_x_bf16_kernel", "rownorm_bf16_kernel", "prep_wnorm_kernel", "debug_mfma16_kernel"}


def base_name(mangled):
    m = re.match(r"_ZN6somhip(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))]


@pytest.fixture(scope="module")
def kernels():
    _lib.load()                                   # (missing or stale library: fails here, as in every test that calls into it)
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    names = sorted({m.decode("ascii")[:-3] for m in re.findall(rb"_ZN6somhip\d+\w+\.kd", blob)})
    assert len(names) > 300
    return names


def scan_instances(kernels, base, tag):
    """(feature count, flags) of the instances of a scan kernel with operand type `tag`"""
    got = set()
    for n in kernels:
        m = re.match(r"_ZN6somhip\d+%sILi(\d+)E%s((?:Lb[01]E){3})E" % (base, tag), n)
        if m:
            got.add((int(m.group(1)), m.group(2)))
    return got


def test_no_bf16_instance_of_an_exact_kernel(kernels):
    assert [n for n in kernels if "exact_" in n and "4Bf16" in n] == []


def test_bf16_scan_kernels_are_the_plain_ones(kernels):
    k16 = scan_instances(kernels, "bmu_bf16_k16_kernel", "4Bf16")
    wide = scan_instances(kernels, "bmu_bf16_wide_kernel", "4Bf16")
    assert k16 == {(k, PLAIN) for k in range(1, 5)}
    assert wide == {(k, PLAIN) for k in range(5, 26)}
    # (nothing the pattern above missed)
    assert sum("4Bf16" in n and base_name(n) in ("bmu_bf16_k16_kernel", "bmu_bf16_wide_kernel") for n in kernels) == 4 + 21


def test_f16_side_is_whole(kernels):
    assert scan_instances(kernels, "bmu_bf16_k16_kernel", "3F16") == {(k, v) for k in range(1, 5) for v in K16_VARIANTS}
    assert scan_instances(kernels, "bmu_bf16_wide_kernel", "3F16") == {(k, v) for k in range(5, 26) for v in WIDE_VARIANTS}
    assert any(n.startswith("_ZN6somhip19exact_refine_kernelILi4E3F16") for n in kernels)
    for base in ("exact_plan_fused_kernel", "prep_w_exact_k16_kernel"):
        assert any(base_name(n) == base and "3F16" in n for n in kernels), base


def test_kernels_with_a_bf16_instance(kernels):
    count = collections.Counter(base_name(n) for n in kernels if "4Bf16" in n)
    assert set(count) == BF16_KERNELS, sorted(count.items())
