"""Compares the device assembly of two builds function by function: python scripts/asm_identity.py OLD.s NEW.s OLD.log NEW.log
The .s files come from `make -C cairo_zstd_amd/csrc asm`, the logs are that command's output (the kernel-resource-usage remarks).
__hip_cuid_* and the function index in block labels (BB<n>_, .LJTI<n>_, .Lfunc_end<n>) are normalised: they move when a kernel is
added in the middle of the module.  Prints one line per function of OLD and the resource line of every function only NEW has."""
import re, sys, hashlib
def funcs(path):
    out, name, body = {}, None, []
    rest = []
    for line in open(path):
        line = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', line)
        m = re.match(r'^([A-Za-z_][\w$.]*):\s*; @', line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r'^\.Lfunc_end\d+:', line):
                out[name] = body; name = None
                continue
            line = re.sub(r'BB\d+_', 'BB_', line)
            line = re.sub(r'\.LJTI\d+_', '.LJTI_', line)
            line = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', line)
            body.append(line)
        else:
            rest.append(line)
    return out, rest
def res(log):
    out, name = {}, None
    for line in open(log):
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m: name = m.group(1); out[name] = []; continue
        m = re.search(r'remark:\s+(.*?): (\S+) \[-Rpass', line)
        if m and name: out[name].append((m.group(1), m.group(2)))
    return out
pa, _ = funcs(sys.argv[1]); nb, _ = funcs(sys.argv[2])
ra, rb = res(sys.argv[3]), res(sys.argv[4])
print(f"functions: parent {len(pa)}, this commit {len(nb)}")
same = 0
for k in pa:
    if k not in nb: print("MISSING", k); continue
    a, b = pa[k], nb[k]
    ins = sum(1 for l in a if l.startswith('\t') and not l.startswith('\t.') and not l.startswith('\t;'))
    ok = a == b
    same += ok
    print(f"  {'identical' if ok else 'DIFFERENT'}  {ins:6d} instructions  sha256 {hashlib.sha256(''.join(a).encode()).hexdigest()[:16]}  {k}")
    if ra.get(k) != rb.get(k): print("    RESOURCE LINE DIFFERS", ra.get(k), rb.get(k))
print(f"{same} of {len(pa)} pre-existing functions identical")
for k in nb:
    if k not in pa:
        print("new:", k, ' '.join(f"{a}={b}" for a, b in rb.get(k, [])))
