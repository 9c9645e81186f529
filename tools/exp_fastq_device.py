"""Diagnostic: the figures of DESIGN 5 "FASTQ text parsed on the device", on bench.py --full's from_file workload (2 M reads of
150 bp as plain FASTQ, 627 MB):
1. the drop-in (new_or_append_hopo_counter_from_file + finalise_hopo_counter) under TATAJUBA_AMD_FASTQ_PARSE=host and =device,
   in alternating runs within this process, at TATAJUBA_AMD_FEEDER_THREADS 16 and 2: seconds and reads per second of each run,
   every run's kept records and index compared with the first run's;
2. the parse kernels alone on the text resident in HBM (tjamd_fastq_push_device in pieces of 64 MiB, parse only):
   tjamd_last_fastq_ms and the text bytes per second, beside a device copy of the same bytes.
   python tools/exp_fastq_device.py [--reads N] [--resources]
--resources: compile tatajuba_amd/csrc/hopo_device.hip with -Rpass-analysis=kernel-resource-usage (no GPU needed) and print the
table of the parse kernels."""
import ctypes, hashlib, os, re, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def resources():
    src = os.path.join(ROOT, "tatajuba_amd", "csrc", "hopo_device.hip")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ", "")}
            rows.append(cur)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split()[0]] = int(m.group(2))
    print(f"{'kernel':42s} SGPRs VGPRs scratch waves/SIMD LDS")
    for row in rows:
        if re.match(r"fq_", row["name"]):
            print(f"{row['name']:42s} {row['TotalSGPRs']:5d} {row['VGPRs']:5d} {row['ScratchSize']:7d} {row['Occupancy']:10d} {row['LDS']:6d}")

if "--resources" in sys.argv:
    resources()
    sys.exit(0)

import torch
import tatajuba_amd as tj

n_reads = int(sys.argv[sys.argv.index("--reads") + 1]) if "--reads" in sys.argv else 2_000_000
K, M, COV, L = 10, 3, 5, 150
host = tj.synth_stream(n_reads, L, 5_000_000)
reads = bytes(host).split(b"\n")[:-1]
tmp = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
fq = os.path.join(tmp, "bench.fq")
with open(fq, "wb") as f:
    for i in range(0, len(reads), 100000):
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (j, reads[j], b"I" * len(reads[j])) for j in range(i, min(len(reads), i + 100000))))
size = os.path.getsize(fq)
print(f"{len(reads)} reads of {L} bp, {size / 1e6:.0f} MB of FASTQ text", flush=True)
L_ = tj.lib()
L_.tjamd_debug_fastq_sessions.restype = ctypes.c_long

# 1. the drop-in, host and device alternating
opt = tj.Options.defaults(K, M, COV, True)
first = None
for threads in (16, 2):
    os.environ["TATAJUBA_AMD_FEEDER_THREADS"] = str(threads)
    times = {"host": [], "device": []}
    for rep in range(4):
        for mode in ("host", "device"):
            os.environ["TATAJUBA_AMD_FASTQ_PARSE"] = mode
            before = L_.tjamd_debug_fastq_sessions()
            t = time.perf_counter()
            h = tj.HopoCounter.new_or_append_from_file(None, fq, opt)
            n_raw = h.c.n_elem
            h.finalise()
            dt = time.perf_counter() - t
            gi, gf = h.idx()
            sig = (n_raw, h.c.n_elem, h.c.n_idx, h.c.coverage, hashlib.sha256(h.elems().tobytes() + gi.tobytes() + gf.tobytes()).hexdigest())
            h.delete()
            first = first or sig
            assert sig == first, (threads, mode, rep, sig, first)                   # the same kept records, index and coverage as the first run
            assert L_.tjamd_debug_fastq_sessions() - before == (1 if mode == "device" else 0)
            times[mode].append(dt)
    for mode in ("host", "device"):
        v = np.array(times[mode][1:])                                                # (the first run of each also pins its buffers)
        print(f"[drop-in, {threads:2d} feeder threads, {mode:6s}] {np.median(v) * 1e3:7.1f} ms ({v.min() * 1e3:.1f}-{v.max() * 1e3:.1f}), "
              f"{len(reads) / np.median(v) / 1e6:6.1f} M reads/s, {size / np.median(v) / 1e9:5.2f} GB/s of text; first run {times[mode][0] * 1e3:.1f} ms", flush=True)
print(f"every run kept the same records: raw {first[0]}, kept {first[1]}, contexts {first[2]}, coverage {first[3]}", flush=True)
del os.environ["TATAJUBA_AMD_FASTQ_PARSE"], os.environ["TATAJUBA_AMD_FEEDER_THREADS"]

# 2. the parse kernels on text resident in HBM, beside a device copy
text = torch.from_numpy(np.fromfile(fq, dtype=np.uint8)).cuda()
other = torch.empty_like(text)
PIECE = 64 << 20
c = tj.Counter(K)
ms = []
for rep in range(6):
    c.fastq_begin(-1)
    for at in range(0, size, PIECE):
        c.fastq_push_device(text.data_ptr() + at, min(PIECE, size - at), final=(at + PIECE >= size))
    consumed, n, stop, n_stream = c.fastq_end()
    assert (consumed, n, stop, n_stream) == (size, len(reads), 0, host.size), (consumed, n, stop, n_stream)
    ms.append(c.last_fastq_ms())
got = c.fastq_stream()
assert got == bytes(host), "the parsed stream differs from the reads"
v = np.array(ms[1:])
cp = []
for rep in range(6):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); other.copy_(text); e1.record(); torch.cuda.synchronize()
    cp.append(e0.elapsed_time(e1))
w = np.array(cp[1:])
n_push = (size + PIECE - 1) // PIECE
print(f"[parse kernels, {n_push} pushes of 64 MiB] {np.median(v):.3f} ms ({v.min():.3f}-{v.max():.3f}), {size / np.median(v) / 1e6:.0f} GB/s of text; "
      f"a device copy of the same bytes {np.median(w):.3f} ms ({w.min():.3f}-{w.max():.3f}), {size / np.median(w) / 1e6:.0f} GB/s", flush=True)
c.close()
os.remove(fq); os.rmdir(tmp)
