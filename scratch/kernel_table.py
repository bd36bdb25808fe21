"""Register, scratch, LDS and code-byte table of every kernel of some HIP sources, here against another checkout of the repository
(usually the parent commit):
    python scratch/kernel_table.py --parent DIR ortk_attn.hip ortk_decode.hip
Each source is compiled for the device alone (`hipcc -O3 --offload-arch=gfx950 --cuda-device-only -c`) in both trees with
`-Rpass-analysis=kernel-resource-usage`; the registers, scratch and static LDS bytes are the compiler's remarks, the code bytes the
size of the kernel's symbol in the code object, and `same code` says whether the disassembly of the symbol (encodings included,
addresses removed) is the parent's.  Kernels are listed and matched by their demangled names (a trailing `false` template argument dropped); one that exists only here
is `new`.  No GPU needed."""
import argparse, hashlib, os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("sparse-image-captioning_amd", "csrc")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
KEYS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"))


def demangle(names):
    """mangled -> demangled name without the parameter list; a trailing `false` template argument is dropped, so that an instance
    keeps its name when its template gains a compile-time switch that defaults to off"""
    # (binutils' c++filt does not know DF16b, the bf16 type: it travels as `half`)
    out = subprocess.run(["c++filt"] + [n.replace("DF16b", "Dh") for n in names], capture_output=True, text=True)
    dem = [d.replace("half", "bf16") for d in out.stdout.splitlines()] if out.returncode == 0 else names
    clean = []
    for d in dem:
        d = re.sub(r"^void ", "", d.replace("(anonymous namespace)::", ""))
        d = re.sub(r"\(ortk_attn_args.*$|\(.*\)$", "", d)
        clean.append(re.sub(r", false>$", ">", d))
    return dict(zip(names, clean))


def kernels(root, src, tmp):
    obj = os.path.join(tmp, os.path.basename(root.rstrip("/")) + "_" + src + ".o")
    r = subprocess.run([os.environ.get("HIPCC", "hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-Wno-pass-failed",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj], cwd=os.path.join(root, CSRC), capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-3000:])
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    sym = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", obj], capture_output=True, text=True, check=True).stdout
    for line in sym.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[7] in res:
            res[f[7]]["bytes"] = int(f[2])
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], capture_output=True, text=True, check=True).stdout
    cur = None
    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = res.get(m.group(1))
            if cur is not None:
                cur["h"] = hashlib.sha1()
        elif cur is not None and line.strip():
            # "\tinstruction operands   // address: encoding": keep the encoding, drop the address and the operands' symbolic targets
            enc = line.split("//")[-1].split(":", 1)[-1].strip() if "//" in line else line.strip()
            cur["h"].update(enc.encode())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="checkout of the commit to compare against")
    ap.add_argument("sources", nargs="+")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        for src in a.sources:
            here = kernels(HERE, src, tmp)
            par = kernels(a.parent, src, tmp) if os.path.exists(os.path.join(a.parent, CSRC, src)) else {}      # (a source the parent does not have)
            names = demangle(sorted(set(here) | set(par)))
            here, par = {names[n]: v for n, v in here.items()}, {names[n]: v for n, v in par.items()}
            names = {n: n for n in set(here) | set(par)}
            print(f"---- {src}: kernel | " + " | ".join(k for _, k in KEYS) + " | code bytes | against the parent")
            for mangled in sorted(here, key=lambda n: names[n]):
                k = here[mangled]
                row = [k.get(key, "?") for key, _ in KEYS] + [str(k.get("bytes", "?"))]
                if mangled not in par:
                    verdict = "new"
                else:
                    p = par[mangled]
                    diff = [short for key, short in KEYS if p.get(key) != k.get(key)]
                    if p.get("bytes") != k.get("bytes"):
                        diff.append(f"code bytes (parent {p.get('bytes')})")
                    same = "h" in p and "h" in k and p["h"].hexdigest() == k["h"].hexdigest()
                    verdict = ("same resources, " + ("same code" if same else "encodings differ")) if not diff else "DIFFERS: " + ", ".join(diff)
                print(f"{names[mangled]} | " + " | ".join(row) + f" | {verdict}")
            print("kernels of the parent missing here:", sorted(names[n] for n in par if n not in here))


if __name__ == "__main__":
    main()
