// snarkjs_amd/js/device_queue.js — ONE queue in front of the device for every fused prover of this process (groth16_native.js, plonk_native.js,
// fflonk_native.js: everything registerAll(snarkjs, { fused: true }) installs).
//
// The library keeps the results of work that is enqueued and not yet collected in per-slot host state (include/zkmi.h, zkmi_pipeline_select): the pinned window
// sums of a Groth16 proof in flight, of the commitments of a PLONK / FFLONK round between their enqueue and their collect. Until this module each prover
// serialised only itself, all of them on pipeline slot 0, so `Promise.all([snarkjs.plonk.prove(..), snarkjs.fflonk.prove(..), snarkjs.groth16.prove(..)])`
// interleaved at every await and one proof collected the other's sums. Now there is one holder of the device at a time, served in arrival order:
//
//   exclusive(run)   a host-orchestrated proof (PLONK, FFLONK): `run` is an async function that owns both pipeline slots until its promise settles;
//   pipelined(job)   a Groth16 proof: { key, curveId, witness, r, s, submit, collect, single }. Groth16 requests that are ADJACENT in arrival order share the
//                    two slots exactly as before (submit0 submit1 collect0 submit0 collect1 ...: never more than two in flight, the older one collected
//                    before a third is submitted); a request with no Groth16 neighbour and nothing in flight takes the one-call path (job.single).
//
// Only the head of the queue is ever started, so a waiting request of another protocol is served as soon as the proofs in flight ahead of it are collected:
// a steady stream of Groth16 requests behind it cannot overtake it. A job that fails rejects its own promise only and releases the device.
"use strict";

const queue = [];                                          // arrival order: { kind: "excl", run, resolve, reject } | { kind: "pipe", job }
let pumping = false;

function enqueue(ent) {
    queue.push(ent);
    if (!pumping) { pumping = true; Promise.resolve().then(pump); }            // started behind the current turn: requests made in the same turn are all in the queue when it looks
}
function pipelined(job) {
    return new Promise((resolve, reject) => enqueue({ kind: "pipe", job: Object.assign(job, { resolve, reject }) }));
}
function exclusive(run) {
    return new Promise((resolve, reject) => enqueue({ kind: "excl", run, resolve, reject }));
}

// The synchronous provers (plonk_native.prove / proveMany, fflonk_native.prove) do not pass through this queue: they hold the main thread from their first call to their
// last. A Groth16 call already handed to a libuv pool thread can still run between two of their calls and is then refused by the library (include/zkmi.h: "pipeline slot N
// holds work in flight"). That rejection reaches this thread only after the synchronous proof has returned, so the call is made once more, behind one turn of the event loop.
const SLOT_BUSY = /pipeline slot \d holds work in flight/;
async function overSyncCaller(call) {
    try { return await call(); } catch (e) {
        if (!(e && SLOT_BUSY.test(e.message))) throw e;
        await new Promise((resolve) => setImmediate(resolve));
        return call();
    }
}

async function pump() {
    const flight = [];                                     // Groth16 proofs submitted and not collected: oldest first
    try {
        while (queue.length || flight.length) {
            const head = queue[0];
            if (head && head.kind === "pipe") {
                if (!flight.length && head.job.single && !(queue[1] && queue[1].kind === "pipe")) {
                    // a lone request with nothing in flight: the one-call path (zkmi_groth16_prove) — measured 4 ms faster per isolated proof than submit + collect from Node
                    // (11.1 against 15.2 ms at 2^20); requests that arrive meanwhile wait in the queue and pipeline from the next turn on
                    const job = queue.shift().job;
                    try { job.resolve(await overSyncCaller(() => job.single(job.curveId, job.key, job.witness, job.r, job.s))); } catch (e) { job.reject(e); }
                    continue;
                }
                if (flight.length < 2) {
                    const job = queue.shift().job, slot = flight.length ? 1 - flight[0].slot : 0;
                    try { await overSyncCaller(() => job.submit(job.key, job.witness, slot)); flight.push({ job, slot }); } catch (e) { job.reject(e); }
                    continue;
                }
            }
            if (flight.length) {                           // both slots full, or the head needs the device to itself, or nothing else is waiting: the oldest proof first
                const { job, slot } = flight.shift();
                try { job.resolve(await job.collect(job.curveId, job.key, slot, job.r, job.s)); } catch (e) { job.reject(e); }
                continue;
            }
            const ent = queue.shift();                      // an exclusive job, nothing in flight
            try { ent.resolve(await ent.run()); } catch (e) { ent.reject(e); }
        }
    } finally { pumping = false; }
}

module.exports = { pipelined, exclusive };
