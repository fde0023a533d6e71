"""Which kernels of two `hipcc -S --cuda-device-only` listings have the same instruction text (labels renumbered, comments dropped)?
python scripts/isa_same_kernels.py old.s new.s [renames.txt]  -- used to show that a new variant of a textually included kernel
(lga_apply_pp.inc, lga_filter_grad_pp.inc) left every existing instantiation as it was.  Kernels are matched by mangled name;
renames.txt holds `old-symbol new-symbol` pairs, one per line, for kernels to compare across a change of name or of template
arguments (profiles/r24a_renames.txt).  A kernel of old.s that is neither in new.s nor mapped is reported as `missing`."""
import re,sys
def kernels(path):
    t=open(path).read().split('\n')
    out={}
    i=0
    while i<len(t):
        m=re.match(r'^(_ZN2ga\S+):', t[i])
        if m:
            j=i
            while 's_endpgm' not in t[j]: j+=1
            body=[l for l in t[i+1:j+1] if l.strip() and not l.strip().startswith(';')]
            body=[l.split(';')[0].rstrip() for l in body]
            body=[re.sub(r'\.(LBB|Ltmp|LJTI|Lfunc_\w+)\d+(_\d+)?', r'.\1', l) for l in body]
            out[m.group(1)]=body
            i=j
        i+=1
    return out
a=kernels(sys.argv[1]); b=kernels(sys.argv[2])
renames=dict(l.split() for l in open(sys.argv[3]) if l.strip() and not l.startswith('#')) if len(sys.argv)>3 else {}
same=diff=renamed=0
for k in a:
    n=k if k in b else renames.get(k)
    if n not in b: print('missing', k[:60]); continue
    renamed+=n!=k
    if a[k]==b[n]: same+=1
    else:
        diff+=1
        d=[(x,y) for x,y in zip(a[k],b[n]) if x!=y][:2]
        print('DIFF', k[:70], len(a[k]), len(b[n]), d)
print('same',same,'diff',diff,'renamed',renamed,'new',len(set(b)-set(a)-{renames.get(k) for k in a}))
