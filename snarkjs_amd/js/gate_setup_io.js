// snarkjs_amd/js/gate_setup_io.js — the byte helpers and the file reads that plonk_setup_native.js and fflonk_setup_native.js share: little-endian
// integers, the headers of a ptau and of an r1cs file (through a reader of groth16_native.js) and the writer of a key's sections.
"use strict";

function leToBig(b) { let v = 0n; for (let i = b.length - 1; i >= 0; i--) v = (v << 8n) | BigInt(b[i]); return v; }
function bigToLe(v, n) { const o = new Uint8Array(n); for (let i = 0; i < n; i++) { o[i] = Number(v & 0xffn); v >>= 8n; } return o; }
function u32(v) { const b = Buffer.alloc(4); b.writeUInt32LE(v >>> 0); return b; }
// src/misc.js log2 on a 32-bit value
function log2(v) { return v > 0 ? 31 - Math.clz32(v) : 0; }

// section 1 of a ptau file: the base field's prime and the ceremony's power
function readPtauHeader(pt, sp) {
    const h = pt.read(sp[1][0].pos, sp[1][0].len), hv = new DataView(h.buffer, h.byteOffset, h.byteLength);
    const n8 = hv.getUint32(0, true);
    return { q: leToBig(h.subarray(4, 4 + n8)), power: hv.getUint32(4 + n8, true) };
}

// section 1 of an r1cs file
function readR1csHeader(r1, sr) {
    const h = r1.read(sr[1][0].pos, sr[1][0].len), hv = new DataView(h.buffer, h.byteOffset, h.byteLength);
    const n8 = hv.getUint32(0, true);
    return { n8, prime: leToBig(h.subarray(4, 4 + n8)), nVars: hv.getUint32(4 + n8, true), nOutputs: hv.getUint32(8 + n8, true),
             nPubInputs: hv.getUint32(12 + n8, true), nConstraints: hv.getUint32(28 + n8, true) };
}

// createBinFile("zkey", 1, nSections): sec(id, body) appends a section, in the order of the calls; bytes() is the whole file
function zkeyWriter(nSections) {
    const parts = [Buffer.from("zkey"), u32(1), u32(nSections)];
    return {
        sec(id, body) { const l = Buffer.alloc(8); l.writeBigUInt64LE(BigInt(body.length)); parts.push(u32(id), l, body); },
        bytes() { return new Uint8Array(Buffer.concat(parts)); },
    };
}

module.exports = { leToBig, bigToLe, u32, log2, readPtauHeader, readR1csHeader, zkeyWriter };
