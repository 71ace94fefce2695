"""Compare the device code of two builds function by function: python tools/device_code_diff.py PARENT.s BRANCH.s, where each
file is the gfx950 assembly of csrc/ofdg_api.hip (the Makefile's flags plus --offload-device-only -S -cuid=ofdg).  A function
is its instruction stream (label to .Lfunc_end) and its .amdhsa_kernel block, with the numbers of local labels (.LBB<n>_,
.Lfunc_end<n>, .Ltmp<n>; BB<n>_ in the loop comments too) taken out: they count functions, so a new one renumbers those
behind it.  Prints how many functions of
the parent are identical in the branch, which differ or are missing, and which are new."""
import re, sys, hashlib
def functions(path):
    """name -> normalised text of the function body (label .. .Lfunc_end) and of its .amdhsa_kernel block"""
    out, cur, name = {}, None, None
    kd = {}
    lines = open(path).read().split("\n")
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"^(_Z\w+|\w+):\s*; @", ln)
        if m and cur is None:
            name, cur = m.group(1), []
        elif cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                out[name] = "\n".join(cur); cur = None
            else:
                cur.append(ln)
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", ln)
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]: j += 1
            kd[m.group(1)] = "\n".join(lines[i:j + 1]); i = j
        i += 1
    norm = lambda t: re.sub(r"BB\d+_", "BB_",re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", re.sub(r"\.Ltmp\d+", ".Ltmp", t)))
    return {k: hashlib.sha256((norm(v) + "\n" + norm(kd.get(k, ""))).encode()).hexdigest() for k, v in out.items()}, {k: v.count("\n") + 1 for k, v in out.items()}
a, la = functions(sys.argv[1]); b, lb = functions(sys.argv[2])
same = [k for k in a if k in b and a[k] == b[k]]
diff = [k for k in a if k in b and a[k] != b[k]]
gone = [k for k in a if k not in b]
new = [k for k in b if k not in a]
print("parent: %d device functions; branch: %d" % (len(a), len(b)))
print("identical instruction stream and kernel descriptor: %d of %d" % (len(same), len(a)))
print("different: %s" % (diff or "none")); print("missing from the branch: %s" % (gone or "none"))
h = hashlib.sha256("".join(sorted(a[k] for k in same)).encode()).hexdigest()
print("sha256 over the %d identical functions' hashes (sorted): %s" % (len(same), h))
print("new in the branch (%d):" % len(new))
for k in new: print("  %s  %d lines" % (k, lb[k]))
