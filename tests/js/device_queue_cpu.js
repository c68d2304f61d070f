// tests/js/device_queue_cpu.js — snarkjs_amd/js/device_queue.js alone, with fake jobs (timers, no addon, no device): arrival order, one holder at a time, the
// two-slot sharing of adjacent Groth16 requests, the lone-request path, release on rejection, and no starvation of another protocol's request behind a Groth16 stream.
// Run:  node tests/js/device_queue_cpu.js
"use strict";
const path = require("path");
const { pipelined, exclusive } = require(path.join(__dirname, "..", "..", "snarkjs_amd", "js", "device_queue.js"));
let fails = 0;
const check = (name, ok) => { if (!ok) { fails++; console.log("FAIL", name); } else console.log("ok  ", name); };
const tick = (ms) => new Promise((res) => setTimeout(res, ms));

// The fake device: a log of what was started and finished, and the invariants the real one needs — a slot holds one proof at a time, and an exclusive job
// runs with nothing in flight and no other exclusive job running.
const log = [], inSlot = [null, null];
let exclRunning = 0, violations = 0;
const busy = () => inSlot[0] !== null || inSlot[1] !== null;
function g16(name, opts) {
    opts = opts || {};
    return {
        key: name, curveId: 0, witness: null, r: null, s: null,
        submit: async (key, w, slot) => {
            if (exclRunning || inSlot[slot] !== null) violations++;
            if (opts.failSubmit) { log.push("submitfail:" + name); await tick(1); throw new Error("submit " + name); }
            inSlot[slot] = name; log.push("submit" + slot + ":" + name); await tick(2);
        },
        collect: async (cid, key, slot) => {
            if (exclRunning || inSlot[slot] !== name) violations++;
            log.push("collect" + slot + ":" + name); await tick(3); inSlot[slot] = null;
            if (opts.failCollect) throw new Error("collect " + name);
            return name;
        },
        single: opts.noSingle ? null : async () => {
            if (exclRunning || busy()) violations++;
            inSlot[0] = name; log.push("single:" + name); await tick(3); inSlot[0] = null;
            return name;
        },
    };
}
function excl(name, opts) {
    opts = opts || {};
    return async () => {
        if (exclRunning || busy()) violations++;
        exclRunning++; log.push("begin:" + name);
        for (let i = 0; i < 3; i++) await tick(1);          // a host-orchestrated proof: several awaits with the device held
        exclRunning--; log.push("end:" + name);
        if (opts.fail) throw new Error("excl " + name);
        return name;
    };
}
const settle = (ps) => Promise.all(ps.map((p) => p.then((v) => ({ v }), (e) => ({ e: e.message }))));
const seqOf = (re) => log.filter((x) => re.test(x)).map((x) => x.split(":")[0]).join(" ");

(async () => {
    // 1. Groth16 alone: the orders tests/js/native_glue.js pins (five and four requests in one turn), a lone request takes the one-call path
    let out = await settle([0, 1, 2, 3, 4].map((i) => pipelined(g16("g" + i))));
    check("five Groth16 requests: two slots, arrival order: " + seqOf(/^(submit|collect)/),
          seqOf(/^(submit|collect)/) === "submit0 submit1 collect0 submit0 collect1 submit1 collect0 submit0 collect1 collect0" && out.map((x) => x.v).join() === "g0,g1,g2,g3,g4");
    log.length = 0;
    out = await settle([0, 1, 2, 3].map((i) => pipelined(g16("h" + i))));
    check("four Groth16 requests: " + seqOf(/^(submit|collect)/), seqOf(/^(submit|collect)/) === "submit0 submit1 collect0 submit0 collect1 submit1 collect0 collect1");
    log.length = 0;
    out = await settle([pipelined(g16("lone"))]);
    check("a lone Groth16 request takes the one-call path", log.join(" ") === "single:lone" && out[0].v === "lone");
    log.length = 0;
    out = await settle([pipelined(g16("nosingle", { noSingle: true }))]);
    check("... and submit + collect when the addon has no one-call entry", log.join(" ") === "submit0:nosingle collect0:nosingle");

    // 2. mixed protocols, one turn: arrival order, one holder at a time; a Groth16 request between two exclusive jobs has no neighbour: one-call path; adjacent ones share the slots
    log.length = 0;
    out = await settle([exclusive(excl("P0")), pipelined(g16("a")), exclusive(excl("F0")), pipelined(g16("b")), pipelined(g16("c")), exclusive(excl("P1")), pipelined(g16("d"))]);
    check("mixed queue, arrival order: " + log.join(" "),
          log.join(" ") === "begin:P0 end:P0 single:a begin:F0 end:F0 submit0:b submit1:c collect0:b collect1:c begin:P1 end:P1 single:d");
    check("every mixed job resolved to its own result", out.map((x) => x.v).join() === "P0,a,F0,b,c,P1,d");

    // 3. requests that arrive while the device is held keep their order
    log.length = 0;
    const first = exclusive(excl("P2"));
    await tick(1);                                           // P2 is running now
    const later = [pipelined(g16("e")), exclusive(excl("F1")), pipelined(g16("f"))];
    out = await settle([first].concat(later));
    check("arrivals during an exclusive job: " + log.join(" "), log.join(" ") === "begin:P2 end:P2 single:e begin:F1 end:F1 single:f");

    // 4. a job that fails rejects only itself and releases the device: exclusive, submit, collect
    log.length = 0;
    out = await settle([exclusive(excl("bad", { fail: true })), pipelined(g16("g")), pipelined(g16("s", { failSubmit: true })), pipelined(g16("c", { failCollect: true })),
                        pipelined(g16("k")), exclusive(excl("P3"))]);
    check("failures stay local: " + JSON.stringify(out.map((x) => x.v || x.e)),
          JSON.stringify(out.map((x) => x.v || x.e)) === JSON.stringify(["excl bad", "g", "submit s", "collect c", "k", "P3"]));
    check("... and the device was released each time: " + log.join(" "), inSlot[0] === null && inSlot[1] === null && exclRunning === 0 && log[log.length - 1] === "end:P3");
    log.length = 0;
    out = await settle([pipelined(g16("after")), exclusive(excl("P4"))]);
    check("the queue is usable after the failures", out.map((x) => x.v).join() === "after,P4");

    // 4b. a call refused because a SYNCHRONOUS prover held the slot (the library's busy-slot error) is made once more behind a turn of the event loop; twice is an error
    log.length = 0;
    const refusing = (name, times) => {
        const j = g16(name), submit = j.submit, single = j.single;
        let left = times;
        const refuse = (f) => async (...a) => { if (left-- > 0) { log.push("refused:" + name); throw new Error("zkmi error 2: groth16: pipeline slot 0 holds work in flight (collect it first)"); } return f(...a); };
        j.submit = refuse(submit); j.single = refuse(single);
        return j;
    };
    out = await settle([pipelined(refusing("r1", 1))]);
    check("one busy-slot refusal of the one-call path is retried: " + log.join(" "), log.join(" ") === "refused:r1 single:r1" && out[0].v === "r1");
    log.length = 0;
    out = await settle([pipelined(refusing("r2", 1)), pipelined(g16("r3")), pipelined(refusing("r4", 2)), exclusive(excl("P5"))]);
    check("... and of a submit; a second refusal rejects that job alone: " + log.join(" "),
          out[0].v === "r2" && out[1].v === "r3" && /holds work in flight/.test(out[2].e || "") && out[3].v === "P5" && inSlot[0] === null && inSlot[1] === null);

    // 5. no starvation: 20 Groth16 jobs queued, one PLONK job arrives third, and a Groth16 stream keeps arriving while it waits
    log.length = 0;
    const ps = [];
    for (let i = 0; i < 20; i++) { if (i === 2) ps.push(exclusive(excl("PLONK"))); ps.push(pipelined(g16("q" + i))); }
    const feeder = (async () => { for (let i = 0; i < 10; i++) { await tick(1); ps.push(pipelined(g16("late" + i))); } })();
    await feeder;
    out = await settle(ps);
    const at = log.indexOf("begin:PLONK"), before = log.slice(0, at), started = (x) => /^(submit|single)/.test(x);
    check("PLONK arriving third is served after the two proofs ahead of it, before the 18 behind: " + before.join(" "),
          before.join(" ") === "submit0:q0 submit1:q1 collect0:q0 collect1:q1" && log[at + 1] === "end:PLONK");
    check("all 31 jobs resolved, Groth16 in arrival order", out.every((x) => x.v) && log.filter(started).map((x) => x.split(":")[1]).join() ===
          Array.from({ length: 20 }, (_, i) => "q" + i).concat(Array.from({ length: 10 }, (_, i) => "late" + i)).join());
    check("after the PLONK job the Groth16 stream shares the two slots again", /submit0:q2 submit1:q3 collect0:q2 submit0:q4 collect1:q3/.test(log.join(" ")));

    check("no invariant of the fake device was ever broken (one proof per slot, exclusive jobs alone)", violations === 0);
    console.log(fails ? `${fails} FAILED` : "ALL OK");
    process.exit(fails ? 1 : 0);
})().catch((e) => { console.log("ERROR", e); process.exit(2); });
