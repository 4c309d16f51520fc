"""Digest of the gfx950 code of every kernel in the given .hip files (no GPU needed): is a move of code a pure move?

    python scripts/kernel_isa_digest.py FILE.hip ... [--save OUT.json] [--against BEFORE.json]

Each file is compiled with the product's flags plus --cuda-device-only -S (a .s file is read as it is).  Per kernel
symbol: sha256 of its body (comments stripped, local label numbers normalised) and of its .amdhsa_* descriptor lines
(registers, LDS, scratch).  --against compares with a saved run and exits 1 unless the two agree exactly.
"""
import hashlib, json, os, re, subprocess, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ferreus_rbf_rs_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "--offload-arch=gfx950"]
LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+")


def assembly(path):
    if path.endswith(".s"):
        return open(path).read(), 0.0
    with tempfile.TemporaryDirectory() as tmp:
        out, t0 = os.path.join(tmp, "a.s"), time.time()
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["--cuda-device-only", "-S", path, "-o", out])
        return open(out).read(), time.time() - t0


def digests(text):
    """{kernel symbol: digest}: the lines from `symbol:` to its .Lfunc_end, and its .amdhsa_kernel block"""
    lines = [l.split(";")[0].strip() for l in text.split("\n")]
    lines = [LABEL.sub(lambda m: "." + m.group(1), l) for l in lines if l]  # .LBB12_3 -> .LBB_3: the function's number goes
    at = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    found = {}
    for i, l in enumerate(lines):
        if l.startswith(".amdhsa_kernel "):
            sym, b = l.split()[1], at[l.split()[1]]
            body = lines[b:lines.index(".Lfunc_end:", b)]
            found[sym] = hashlib.sha256("\n".join(body + lines[i:lines.index(".end_amdhsa_kernel", i)]).encode()).hexdigest()
    return found


if __name__ == "__main__":
    args, opt = [a for a in sys.argv[1:] if not a.startswith("--")], {}
    for flag in ("--save", "--against"):
        if flag in sys.argv:
            opt[flag] = sys.argv[sys.argv.index(flag) + 1]
            args.remove(opt[flag])
    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "16"))) as pool:
        units = list(pool.map(assembly, args))
    merged, twice = {}, []
    for path, (text, seconds) in zip(args, units):
        d = digests(text)
        twice += sorted(set(d) & set(merged))
        merged.update(d)
        print(f"{os.path.basename(path)}: {len(d)} kernels, compiled in {seconds:.0f} s")
    for sym in sorted(merged):
        print(merged[sym][:16], sym)
    if "--save" in opt:
        json.dump(merged, open(opt["--save"], "w"), indent=0, sort_keys=True)
    before = json.load(open(opt["--against"])) if "--against" in opt else merged
    differ = [s for s in set(merged) & set(before) if merged[s] != before[s]]
    print(f"SUMMARY {len(merged)} kernels ({len(before)} before), {len(twice)} in two files, {len(set(before) - set(merged))} missing, "
          f"{len(set(merged) - set(before))} new, {len(differ)} with a different digest")
    sys.exit(1 if twice or differ or set(before) != set(merged) else 0)
