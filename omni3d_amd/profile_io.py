"""Small helpers of the benchmark reports: rows of the committed rocprofv3 PMC summaries (profiles/*.csv, written by
tools/pmc_run.py) and a counter of the multiply-adds the MFMA launchers actually execute in one step."""
import csv
import hashlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def profile_counters(csv_name, kernel_substr, grid=None):
    """Row of a committed PMC summary for one kernel (+ the file's sha256).  Counters cannot be collected inside a normal bench
    run (the --pmc passes serialise the kernels), so the bench JSON quotes the tracked table it takes them from."""
    path = os.path.join(ROOT, "profiles", csv_name)
    if not os.path.exists(path):
        return None
    digest = hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]
    rows = [r for r in csv.DictReader(open(path)) if kernel_substr in r["kernel"] and (grid is None or int(float(r["grid"])) == grid)]
    if not rows:
        return None
    r = max(rows, key=lambda q: float(q.get("GRBM_GUI_ACTIVE", "0") or 0))

    def f(k):
        try:
            v = float(r[k])
            return v if v == v else None
        except (KeyError, ValueError):
            return None
    out = {"source": f"profiles/{csv_name}", "sha256_16": digest, "kernel": r["kernel"], "grid": int(float(r["grid"]))}
    for k in ("FETCH_SIZE_x2_MB", "WRITE_SIZE_MB", "SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE", "SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_VALU",
              "SQ_INSTS_VALU", "SQ_THREAD_CYCLES_VALU", "SQ_WAIT_INST_ANY", "SQ_WAIT_ANY", "SQ_BUSY_CYCLES", "mfma_flop"):
        out[k] = f(k)
    # cycle-based (DVFS-independent) MFMA utilisation: busy SIMD-cycles / (GUI-active cycles per XCD x 1024 SIMDs); GRBM_GUI_ACTIVE is
    # summed over the 8 XCDs on gfx950 (profiles/README.md)
    if out["SQ_VALU_MFMA_BUSY_CYCLES"] and out["GRBM_GUI_ACTIVE"]:
        out["mfma_busy_frac"] = out["SQ_VALU_MFMA_BUSY_CYCLES"] / (out["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0)
    if out["SQ_ACTIVE_INST_VALU"] and out["SQ_WAVE_CYCLES"]:
        out["valu_active_frac_of_wave_cycles"] = out["SQ_ACTIVE_INST_VALU"] / out["SQ_WAVE_CYCLES"]
    # share of the chip's SIMD-cycles with a VALU instruction in flight (the SQ_* counters are in quad-cycles, MI355X_MICROARCH.md):
    # the figure of merit of a VALU-issue-bound kernel (IoU3D), as VERDICT r4 recomputed it from the committed counters
    if out["SQ_ACTIVE_INST_VALU"] and out["GRBM_GUI_ACTIVE"]:
        out["valu_busy_frac_of_simd_cycles"] = out["SQ_ACTIVE_INST_VALU"] * 4.0 / (out["GRBM_GUI_ACTIVE"] / 8.0 * 1024.0)
    # average share of a wave's 64 lanes that are active in a VALU instruction (thread-cycles per instruction / 64)
    if out.get("SQ_THREAD_CYCLES_VALU") and out["SQ_INSTS_VALU"]:
        out["valu_lane_utilisation"] = out["SQ_THREAD_CYCLES_VALU"] / (64.0 * out["SQ_INSTS_VALU"])
    return out


def latest_profile(name, rounds=("r06", "r05", "r04", "r03", "r02")):
    """newest committed round of a profile artefact: profiles/r06_<name> if it exists, else r05_<name>, ..."""
    for r in rounds:
        if os.path.exists(os.path.join(ROOT, "profiles", f"{r}_{name}")):
            return f"{r}_{name}"
    return f"{rounds[0]}_{name}"


class ExecutedFlops:
    """`with ExecutedFlops() as c:` counts 2 x multiply-adds of every MFMA launch made through the C ABI (direct convolutions at
    their implicit-GEMM size, Winograd layers at the size of their point GEMMs, FC GEMMs) -- the EXECUTED flops, as opposed to
    the algorithmic (direct-convolution) count SURVEY.md 8(d) prices the step with."""

    def __enter__(self):
        from . import lib
        self.lib = lib.get()
        self.flops = 0.0
        self.by_entry = {}
        self._orig = self.lib.call

        def call(name, *a):
            f = self._flops(name, a)
            if f:
                self.flops += f
                self.by_entry[name] = self.by_entry.get(name, 0.0) + f
            return self._orig(name, *a)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self._orig
        return False

    @staticmethod
    def _flops(name, a):
        return executed_flops(name, a)


_SIGNATURES = None
MFMA_ENTRY = re.compile(r"conv|gemm|stem|head16")
# entries that match the pattern but run on the VALU (HBM-bound by design): depthwise k x k convolutions (csrc/depthwise.hip), the fused
# RPN head's data / weight gradient (csrc/rpn_head.hip: only its forward is MFMA 16x16x4)
VALU_ENTRIES = frozenset(["omni_dwconv_fwd", "omni_dwconv_dgrad", "omni_dwconv_wgrad", "omni_rpn_head16_dgrad", "omni_rpn_head16_wgrad"])


def abi_signatures():
    """{entry point: [argument names]} of include/omni3d_hip.h"""
    global _SIGNATURES
    if _SIGNATURES is None:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "omni3d_hip.h")).read(), flags=re.S)
        _SIGNATURES = {m.group(1): [x.strip().split()[-1].lstrip("*") for x in " ".join(m.group(2).split()).split(",")]
                       for m in re.finditer(r"\bint\s+(omni_\w+)\s*\(([^)]*)\)\s*;", text)}
    return _SIGNATURES


def flop_class(name):
    """how `executed_flops` prices an entry point: 'conv' | 'conv_multi' | 'conv_s2' | 'grouped' | 'stem' | 'gemm_batched' | 'gemm_batched_multi' | 'engine' |
    'head16' (MFMA launchers), 'valu' (matches the MFMA name pattern but has no MFMA in it), None (not an MFMA launcher).
    tests/test_profile_io.py asserts that every header entry matching conv|gemm|stem|head16 gets a class -- VERDICT r4 weak 8: the
    counter did not know the *_det / *_multi / *_s2 entries the default path had moved to and reported a third of the executed flops."""
    names = abi_signatures().get(name)
    if names is None or not MFMA_ENTRY.search(name):
        return None
    if name in VALU_ENTRIES:
        return "valu"
    if name.startswith("omni_rpn_head16"):
        return "head16"
    if name.startswith("omni_stem_conv"):
        return "stem"
    if name.startswith("omni_gemm_engine"):
        return "engine"
    if name == "omni_gemm_batched_wgrad_multi":
        return "gemm_batched_multi"
    if name.startswith("omni_gemm_batched"):
        return "gemm_batched"
    if name.startswith("omni_grouped_conv2d"):
        return "grouped"
    if name in ("omni_conv2d_fwd_multi_det", "omni_conv2d_wgrad_multi_det"):
        return "conv_multi"
    if name == "omni_conv2d_s2_dgrad":
        return "conv_s2"
    if name.startswith("omni_conv2d"):
        return "conv"
    return None


def _host_ints(ptr, n, ctype):
    import ctypes
    if ptr is None:
        return []
    addr = ptr.value if hasattr(ptr, "value") else int(ptr)
    return list(ctypes.cast(addr, ctypes.POINTER(ctype))[:n])


def executed_flops(name, a):
    """2 x multiply-adds one C-ABI call puts on the matrix cores, from the ARGUMENT NAMES of the header (0 for planning calls of the
    deterministic entry points -- plan != NULL launches nothing -- and for everything that is not an MFMA launcher)"""
    import ctypes
    cls = flop_class(name)
    if cls in (None, "valu"):
        return 0.0
    v = dict(zip(abi_signatures()[name], a))
    if v.get("plan") is not None:
        return 0.0
    if cls in ("conv", "grouped"):
        OH = (v["H"] + 2 * v["pad"] - v["R"]) // v["stride"] + 1
        OW = (v["W"] + 2 * v["pad"] - v["S"]) // v["stride"] + 1
        return 2.0 * v["N"] * OH * OW * v["K"] * v["R"] * v["S"] * v["C"] / (v["groups"] if cls == "grouped" else 1)
    if cls == "conv_multi":       # 1 x 1 convolution over the concatenation of nsrc maps
        return 2.0 * v["N"] * v["H"] * v["W"] * v["K"] * sum(_host_ints(v["cs"], v["nsrc"], ctypes.c_int))
    if cls == "conv_s2":          # 3x3 / stride 2 / pad 1 data gradient
        return 2.0 * v["N"] * ((v["H"] - 1) // 2 + 1) * ((v["W"] - 1) // 2 + 1) * v["K"] * 9 * v["C"]
    if cls == "stem":
        stride = 2 if "_s2_" in name else 1
        OH, OW = (v["H"] - 1) // stride + 1, (v["W"] - 1) // stride + 1
        return 2.0 * v["N"] * OH * OW * v["K"] * v["R"] * v["R"] * v["C"]
    if cls == "gemm_batched":
        if "N" in v and "C" not in v:          # omni_gemm_batched_split (M x N x K naming)
            return 2.0 * v["batch"] * v["M"] * v["N"] * v["K"]
        return 2.0 * v["batch"] * v["M"] * v["C"] * v["K"]
    if cls == "gemm_batched_multi":
        n = v["n"]
        cols = [_host_ints(v[k], n, ctypes.c_int) for k in ("batch", "M", "C", "K")]
        return float(sum(2.0 * b * m * c * k for b, m, c, k in zip(*cols)))
    if cls == "engine":
        return 2.0 * v["batch"] * v["M"] * v["N"] * v["K"]
    if cls == "head16":
        return 2.0 * sum(_host_ints(v["pix"], v["nlev"], ctypes.c_longlong)) * 256 * 16
    return 0.0


def host_cores():
    """what the box's host really offers (SURVEY.md 8d asks for the physical core count next to a CPU baseline): logical CPUs the
    OS shows, CPUs this process may run on, physical cores (distinct (package, core id) pairs of /proc/cpuinfo) and sockets"""
    import os
    info = {"logical_cpus": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
            "physical_cores": None, "sockets": None, "model": None}
    try:
        cores, pk = set(), None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                pk = line.split(":")[1].strip()
            elif line.startswith("core id"):
                cores.add((pk, line.split(":")[1].strip()))
            elif line.startswith("model name") and info["model"] is None:
                info["model"] = line.split(":")[1].strip()
        if cores:
            info["physical_cores"] = len(cores)
            info["sockets"] = len({c[0] for c in cores})
    except OSError:
        pass
    return info


class GpuState:
    """Clock / power / temperature of the device a rank runs on, read from the amdgpu hwmon files of ITS PCI function (the GPU box
    is one tenant of an 8-GPU host: /sys/class/drm shows every card, torch's device properties say which one is ours).  A read is
    four small files (~50 us): `sample()` between the enqueue of a timed window and its synchronize sees the device UNDER the load,
    which is what a step-time difference between two boxes has to be explained with.  `neighbours()`:
    how many of the host's other GPUs are clocked up, and their summed power -- the other tenants share the host's CPUs."""

    FILES = (("sclk_mhz", "freq1_input", 1e-6), ("mclk_mhz", "freq2_input", 1e-6), ("power_w", "power1_input", 1e-6),
             ("temp_junction_c", "temp2_input", 1e-3), ("temp_mem_c", "temp3_input", 1e-3))

    def __init__(self, index=0):
        self.dir, self.hwmon, self.address = None, None, None
        try:
            import glob
            import torch
            p = torch.cuda.get_device_properties(index)
            self.address = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
            d = os.path.join("/sys/bus/pci/devices", self.address)
            hw = sorted(glob.glob(os.path.join(d, "hwmon", "hwmon*")))
            if hw:
                self.dir, self.hwmon = d, hw[0]
        except Exception:  # noqa: BLE001 -- no GPU / no sysfs: every sample is None
            pass

    @staticmethod
    def _read(path, scale):
        try:
            with open(path) as f:
                return round(float(f.read().split()[0]) * scale, 1)
        except (OSError, ValueError, IndexError):
            return None

    def sample(self):
        if self.hwmon is None:
            return None
        out = {k: self._read(os.path.join(self.hwmon, f), s) for k, f, s in self.FILES}
        out["busy_pct"] = self._read(os.path.join(self.dir, "gpu_busy_percent"), 1.0)
        return out

    def neighbours(self):
        """the host's OTHER GPUs: count, how many run above 1 GHz right now, their summed socket power"""
        if self.hwmon is None:
            return None
        import glob
        n = up = 0
        watts = 0.0
        for hw in glob.glob("/sys/bus/pci/devices/*/hwmon/hwmon*"):
            if hw == self.hwmon:
                continue
            try:
                if open(os.path.join(hw, "name")).read().strip() != "amdgpu":
                    continue
            except OSError:
                continue
            n += 1
            f = self._read(os.path.join(hw, "freq1_input"), 1e-6)
            up += 1 if (f or 0) > 1000 else 0
            watts += self._read(os.path.join(hw, "power1_input"), 1e-6) or 0.0
        return {"other_gpus": n, "clocked_up": up, "power_w_sum": round(watts, 0)}
