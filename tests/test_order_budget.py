"""The ordering step's kernels must be able to start on a CU that the scan fills.

scan_fast_kernel<1, true> is persistent: three workgroups of eight wavefronts stay on every CU until the scan ends.  A
sample's ordering step (bin_scan, bin_scatter, bin_sort_index, bin_sort_full, bin_ctx_scan, bin_ctx_write) is queued on a
side stream beside the next sample's scan, and gains nothing unless a workgroup of each of its kernels fits into what those
three leave: one more wavefront per SIMD of at most 32 registers, and some LDS.  This test compiles hopo_device.hip for the
device only, with the Makefile's flags, reads the compiler's resource remarks and asserts both halves: the ordering kernels
keep to their budget without scratch, and the scan kernel still leaves that budget.  It reads resource counts only.  No GPU
is needed (about half a minute of compilation)."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tatajuba_amd", "csrc")

ORDER_KERNELS = ("bin_scan_kernel", "bin_scatter_kernel", "bin_sort_index_kernel", "bin_sort_full_kernel", "bin_ctx_scan_kernel", "bin_ctx_write_kernel")
SCAN_KERNEL = "scan_fast_kernel<1, true>"
SCAN_THREADS, SCAN_WG_PER_CU = 512, 3                       # FK_BLOCK, FK_LOG_WG_PER_CU

# the budget (a gfx950 CU: four SIMDs, 512 registers per lane and eight wavefront slots on each, 160 KiB of LDS; registers
# are handed out in blocks of eight)
REG_BUDGET, LDS_BUDGET, WG_THREADS_MAX = 32, 32768, 256
SIMD_REGS, SIMD_SLOTS, SIMDS, CU_LDS, REG_BLOCK = 512, 8, 4, 160 * 1024, 8
SIMD_SGPRS = 800


def makefile_hipflags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)$", text, re.M).group(1)
    assert arch == "gfx950"
    return flags.replace("$(ARCH)", arch).split()


def mangled_prefix(kernel):
    """the Itanium name of a kernel up to its parameter list: plain functions, and scan_fast_kernel<1, true>"""
    if kernel == SCAN_KERNEL:
        return "_Z16scan_fast_kernelILi1ELb1EE"
    return "_Z%d%s" % (len(kernel), kernel)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel: {field: number}} of the ordering kernels and the scan kernel, from -Rpass-analysis=kernel-resource-usage"""
    out = tmp_path_factory.mktemp("order_budget") / "hopo_device.out"
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc] + makefile_hipflags() + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "hopo_device.hip", "-o", str(out)]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    table, cur, mangled = {}, None, []
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        body = m.group(1)
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            mangled.append(cur)
            table[cur] = {}
        elif cur is not None and ":" in body:
            key, val = body.rsplit(":", 1)
            if re.fullmatch(r"\s*-?\d+\s*", val):
                table[cur][key.strip()] = int(val)
    found = {}
    for kernel in ORDER_KERNELS + (SCAN_KERNEL,):
        hits = [m for m in mangled if m.startswith(mangled_prefix(kernel)) and not m[len(mangled_prefix(kernel))].isdigit()]
        assert len(hits) == 1, (kernel, hits)
        found[kernel] = table[hits[0]]
    return found


def registers(u):
    """what a wavefront of the kernel takes from its SIMD's register file (vector and accumulation registers are one file)"""
    return u["VGPRs"] + u["AGPRs"]


def blocks(n):
    return math.ceil(n / REG_BLOCK) * REG_BLOCK


def scalar_take(u):
    """what a wavefront takes from its SIMD's 800 scalar registers: blocks of 16, and 16 on top"""
    return math.ceil(u["TotalSGPRs"] / 16) * 16 + 16


def test_the_remarks_name_every_kernel_of_the_step(usage):
    for k in ORDER_KERNELS + (SCAN_KERNEL,):
        assert k in usage, (k, sorted(usage)[:20])
        for f in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"):
            assert f in usage[k], (k, f, usage[k])


@pytest.mark.parametrize("kernel", ORDER_KERNELS)
def test_ordering_kernel_keeps_to_its_budget(usage, kernel):
    u = usage[kernel]
    print(kernel, u)
    assert registers(u) <= REG_BUDGET, (kernel, u)
    assert u["LDS Size [bytes/block]"] <= LDS_BUDGET, (kernel, u)
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (kernel, "the budget was met by spilling", u)


@pytest.mark.parametrize("kernel", ORDER_KERNELS)
def test_ordering_kernel_fits_beside_three_scanning_workgroups(usage, kernel):
    s, u = usage[SCAN_KERNEL], usage[kernel]
    scan_waves_per_simd = SCAN_WG_PER_CU * SCAN_THREADS // 64 // SIMDS
    regs_left = SIMD_REGS - scan_waves_per_simd * blocks(registers(s))
    lds_left = CU_LDS - SCAN_WG_PER_CU * s["LDS Size [bytes/block]"]
    print(kernel, "scan:", registers(s), "registers,", s["LDS Size [bytes/block]"], "bytes of LDS; left per SIMD:", regs_left, "registers,", SIMD_SLOTS - scan_waves_per_simd,
          "slots; LDS left:", lds_left)
    # what the scan leaves is the budget the ordering kernels were written to ...
    assert regs_left >= REG_BUDGET, ("scan_fast_kernel<1, true> leaves no wavefront of 32 registers", registers(s), regs_left)
    assert lds_left >= LDS_BUDGET, ("scan_fast_kernel<1, true> leaves less than 32 KiB of LDS", lds_left)
    assert SIMD_SLOTS - scan_waves_per_simd >= 1
    # ... and one workgroup of this kernel, four wavefronts at most, one per SIMD, fits into it
    assert WG_THREADS_MAX // 64 <= SIMDS
    assert blocks(registers(u)) <= regs_left, (kernel, registers(u), regs_left)
    assert u["LDS Size [bytes/block]"] <= lds_left, (kernel, u, lds_left)
    # the scalar registers, which is where it failed on the device while the scan kernel took 106: six wavefronts of 128 left 32
    sgprs_left = SIMD_SGPRS - scan_waves_per_simd * scalar_take(s)
    print(kernel, "scalar registers: scan", s["TotalSGPRs"], "guest", u["TotalSGPRs"], "left per SIMD", sgprs_left)
    assert scalar_take(u) <= sgprs_left, (kernel, u["TotalSGPRs"], s["TotalSGPRs"], sgprs_left)


def test_the_kernels_are_launched_with_workgroups_of_four_wavefronts_at_most():
    """the launch bounds in the source: ORDER_KERNEL states 256 threads, the two sort kernels one wavefront"""
    src = open(os.path.join(CSRC, "hopo_device.hip")).read()
    m = re.search(r"^#define ORDER_KERNEL __launch_bounds__ \((\d+)\)", src, re.M)
    assert m and int(m.group(1)) <= WG_THREADS_MAX
    for k in ORDER_KERNELS:
        head = re.search(r"__global__ ([^\n]*)\nvoid %s \(" % k, src)
        assert head, k
        lb = re.search(r"__launch_bounds__ \((\d+)\)", head.group(1))
        assert "ORDER_KERNEL" in head.group(1) or (lb and int(lb.group(1)) <= WG_THREADS_MAX), (k, head.group(1))
