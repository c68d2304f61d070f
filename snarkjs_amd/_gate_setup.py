"""What plonk_setup.py and fflonk_setup.py share: the call of the library's gate lowering, the device call with the buffers that both protocols
fill, the head of the key's section 2, the X_2 read and the assembly of the key. The twin of csrc/gate_setup.hpp on this side of the C-ABI."""
import ctypes as C
import struct

import numpy as np

from . import zkmi
from .groth16_setup import CURVES, assemble

# getK1K2 (src/plonk_setup.js:484-504) and computeK1K2 (src/fflonk_setup.js:513-532) call Fr.add without assigning its result: they return 2 and 3
# or never return
K1, K2 = 2, 3


def fr_mont(r, v):
    return ((v << 256) % r).to_bytes(32, "little")


def lower(cv, hdr, constraints, fn_len, fn):
    """fn_len / fn: zkmi_plonk_setup_lower_len / zkmi_plonk_setup_lower or their FFLONK twins (host only, need no device): dict plonk_n_vars (nVars of
    the header), n_additions, n_constraints, domain_size and numpy arrays additions (section 3), map_a, map_b, map_c (sections 4 - 6), selectors
    (5 x n_constraints x 32, Montgomery, in the protocol's order), pred (3 x domain_size)"""
    n_public = hdr["nOutputs"] + hdr["nPubInputs"]
    pg = zkmi.pages_of(constraints)
    cnt = (C.c_uint32 * 4)()
    zkmi.check(fn_len(cv["id"], pg.pages, hdr["nConstraints"], hdr["nVars"], n_public, cnt))
    n_vars, n_add, n_c, dom = list(cnt)
    out = dict(plonk_n_vars=n_vars, n_additions=n_add, n_constraints=n_c, domain_size=dom,
               additions=np.zeros(n_add * 72, np.uint8), map_a=np.zeros(n_c, np.uint32), map_b=np.zeros(n_c, np.uint32), map_c=np.zeros(n_c, np.uint32),
               selectors=np.zeros(5 * n_c * 32, np.uint8), pred=np.zeros(3 * dom, np.uint32))
    rec = zkmi.PlonkLowered(n_vars, n_add, n_c, dom, *[out[k].ctypes.data for k in ("additions", "map_a", "map_b", "map_c", "selectors", "pred")])
    zkmi.check(fn(cv["id"], pg.pages, hdr["nConstraints"], hdr["nVars"], n_public, C.byref(rec)))
    return out


def device_sections(cv, n_public, low, points, rec_in, rec_out, fn, extra):
    """One device call (fn: zkmi_plonk_setup or zkmi_fflonk_setup, with its two records): dict q (five arrays: sections 7 - 11), sigma (three
    records), lagrange (max(n_public, 1) records) and the protocol's own outputs, `extra` = (name, bytes) in the order of the output record; numpy uint8"""
    zkmi.init()
    dom = low["domain_size"]
    hold = zkmi.pages_of(points)
    din = rec_in(cv["id"], n_public, low["n_constraints"], dom, low["selectors"].ctypes.data, low["pred"].ctypes.data, hold.pages)
    q = [np.zeros(5 * dom * 32, np.uint8) for _ in range(5)]
    out = {k: np.zeros(n, np.uint8) for k, n in [("sigma", 15 * dom * 32), ("lagrange", max(n_public, 1) * 5 * dom * 32)] + extra}
    dout = rec_out((C.c_void_p * 5)(*[a.ctypes.data for a in q]), *[a.ctypes.data for a in out.values()], q[0].size, *[a.size for a in out.values()])
    zkmi.check(fn(C.byref(din), C.byref(dout)))
    return dict(q=q, **out)


def section2_head(cv, n_public, low):
    """Section 2 from the field sizes and primes through the five counts and k1, k2 (writeHeaders src/plonk_setup.js:436-482, writeFFlonkHeader
    src/fflonk_setup.js:466-503)"""
    q = next(k for k, c in CURVES.items() if c is cv)
    return struct.pack("<I", cv["n8q"]) + q.to_bytes(cv["n8q"], "little") + struct.pack("<I", 32) + cv["r"].to_bytes(32, "little") + \
        struct.pack("<IIIII", low["plonk_n_vars"], n_public, low["domain_size"], low["n_additions"], low["n_constraints"]) + \
        fr_mont(cv["r"], K1) + fr_mont(cv["r"], K2)


def read_x2(ptau, sp, cv):
    """X_2 of the header: the second tauG2 point"""
    s_g2 = 4 * cv["n8q"]
    return ptau.read(sp[3][0][0] + s_g2, s_g2)


def assemble_gate_zkey(sections):
    """createBinFile("zkey", 1, len(sections)) with the sections in the order given, the order in which the reference writes them"""
    data = assemble(sections)
    return data[:8] + struct.pack("<I", len(sections)) + data[12:]
