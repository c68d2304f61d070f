// tools/gen_wtns_check_golden.js — golden verdicts and log lines of snarkjs.wtns.check (snarkjs_amd/wtns_check.py, js/wtns_check_native.js), produced by the
// UNMODIFIED reference on the CPU under a recording logger:
//   python tools/gen_wtns_check_r1cs.py && node --harmony-optional-chaining --harmony-nullish tools/gen_wtns_check_golden.js
// Reads tests/golden/wtns_check_cases.json (name, curve, r1cs file, wtns file, what the case is) and writes tests/golden/wtns_check_golden.json: per case the
// sha256 of its two files, what the call returned or the message it threw, and every logger line with its level; and, per case, what the call does with NO
// logger (a bad witness dies on logger.warn).
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const snarkjs = require(path.join(__dirname, '..', 'oracle', 'ref_shim.js'));
const OUT = path.join(__dirname, '..', 'tests', 'golden');
const sha = b => crypto.createHash('sha256').update(b).digest('hex');

function recorder() {
    const lines = [], push = level => text => lines.push([level, text]);
    return { lines, logger: { debug: push('debug'), log: push('log'), info: push('info'), warn: push('warn'), error: push('error') } };
}
async function attempt(f) {
    const rec = recorder();
    try {
        const r = await f(rec.logger);
        return { returns: r, lines: rec.lines };
    } catch (e) {
        return { throws: e.message, errorName: e.name, lines: rec.lines };
    }
}

(async () => {
    const cases = JSON.parse(fs.readFileSync(path.join(OUT, 'wtns_check_cases.json'), 'utf8'));
    const out = [];
    for (const c of cases) {
        const r1cs = new Uint8Array(fs.readFileSync(path.join(OUT, c.r1cs))), wtns = new Uint8Array(fs.readFileSync(path.join(OUT, c.wtns)));
        const withLogger = await attempt(lg => snarkjs.wtns.check(r1cs, wtns, lg));
        const bare = await attempt(() => snarkjs.wtns.check(r1cs, wtns));
        delete bare.lines;
        out.push(Object.assign({}, c, { r1csSha256: sha(r1cs), wtnsSha256: sha(wtns) }, withLogger, { noLogger: bare }));
        console.log(c.name, '->', withLogger.throws !== undefined ? `throws ${withLogger.errorName}: ${withLogger.throws}` : withLogger.returns, `(${withLogger.lines.length} lines; no logger:`,
                    bare.throws !== undefined ? `throws ${bare.errorName}: ${bare.throws})` : `${bare.returns})`);
    }
    fs.writeFileSync(path.join(OUT, 'wtns_check_golden.json'), JSON.stringify({ reference: 'snarkjs wtns.check, unmodified bundle', cases: out }, null, 1) + '\n');
    process.exit(0);
})().catch(e => { console.error(e); process.exit(1); });
