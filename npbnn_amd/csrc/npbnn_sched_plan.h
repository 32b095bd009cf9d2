/*
 * npbnn_sched_plan.h — the schedule of a device chain's batch as arithmetic on plain numbers: which schedule a batch runs on
 * (npbnn_sched_choose), what the context remembers of the batches before it (npbnn_sched_hist, npbnn_sched_record_*), and how many
 * passes a round launches (npbnn_sched_passes*).  Nothing here touches the GPU, the environment or a launch plan: the caller
 * (chain_prepare and the run entries of npbnn_chain_api.hip) reads those and fills an npbnn_sched_req.  Plain C, so that the host
 * library (npbnn_host.c) exports the same rule the HIP library runs by, for the CPU tests of it (tests/test_host_sched_plan.py).
 */
#ifndef NPBNN_SCHED_PLAN_H
#define NPBNN_SCHED_PLAN_H

#include <math.h>

#include "npbnn_hip.h"

/* NPBNN_SCHED_AUTO between the two persistent forms.  Overlapped (PERSIST): a pass that accepts voids the pass in flight behind it - a
 * decided pass costs (1 + a) turns, a = 1 - (1 - p)^D the share of passes that accept something.  Decision between the passes
 * (PERSIST_SERIAL): no pass in vain, but every turn is longer by the decision and by what the step workgroup cannot hide of preparing
 * the next pass for every outcome - more, the wider the proposals.  The context keeps what an iteration cost on each form
 * (npbnn_sched_hist.it_us: a batch's time over its iterations) and picks the cheaper one; a form that has not run yet is priced from the other
 * one with that model and kSpecTurnExtraUs + kSpecTurnExtraUsPerWeight * M (measured on config-2 shapes: 33.2 against 28.5 us per turn
 * at M = 33, 40 at M = 428), and is given its first batches after kTurnFirstProbeBatches batches on the other when the model puts it within kFirstProbeWithin of it, or after kTurnForcedProbeBatches regardless (then
 * one every kTurnReprobeBatches while within a factor two: measurements go stale).  Short batches (dispatches of 100) and long ones (the
 * sub-batches of a long call) are measured and decided apart. */
static const double kSpecTurnExtraUs = 4.5, kSpecTurnExtraUsPerWeight = 0.0175;
static const double kTurnUsGuess = 30.0;           /* before anything has been measured */
static const int kShortBatch = 256;                /* batches below / from this many iterations are measured (and decided) apart */
static const double kFirstProbeWithin = 1.15;      /* ... if the model prices it within this factor of the measured one (asked again at every batch: the acceptance rate moves) */
static const int kTurnForcedProbeBatches = 200;    /* ... or whatever the model says after this many batches without it (a wrong model must not park a chain for good) */
static const int kTurnFirstProbeBatches = 4;       /* batches on one persistent form before the other, never measured, is given one */
static const int kTurnReprobeBatches = 48;         /* batches on one persistent form before the other's measured turn time is refreshed */
static const int kPersistSerialMaxWidth = 640;     /* ... and the widest proposal (weights perturbed per iteration) it is picked for */
/* slots per value of the evaluating workgroups' tagged sums on NPBNN_SCHED_PERSIST_SERIAL (kSpecPartSlots of npbnn_chain.hip.h, which
 * npbnn_chain_api.hip holds this to) */
#define NPBNN_SCHED_SPEC_PART_SLOTS 256

/* what a context remembers of its batches (npbnn_ctx.sched) */
typedef struct npbnn_sched_hist {
    int last_schedule;         /* schedule of the previous batch */
    int turn_batches[2][2];    /* [form][batch-size class] batches run since that form was last measured in that class (kTurnReprobeBatches) */
    double turn_us[2];         /* measured time of a launch turn (pass, decided or void) of the persistent forms: overlapped, decision between passes */
    int it_n[2][2];            /* [form][batch-size class] batches that went into it_us (the first one of a form is slow: a second follows it) */
    double it_us[2][2];        /* [form][batch-size class] measured time per ITERATION of a batch (what NPBNN_SCHED_AUTO
                                  compares); classes: batches of fewer than kShortBatch iterations, and the others - a form's fixed
                                  cost per batch differs, so what wins in dispatches of 100 need not win in sub-batches of 512 */
    double its_per_pass;       /* iterations a launch decided on average in the previous batch (0: unknown) */
    double accept_rate;        /* acceptance rate of the previous batch (< 0: unknown) */
} npbnn_sched_hist;
#define NPBNN_SCHED_HIST_INIT {0, {{0, 0}, {0, 0}}, {0.0, 0.0}, {{0, 0}, {0, 0}}, {{0.0, 0.0}, {0.0, 0.0}}, 0.0, -1.0}

/* everything the choice reads that is not history */
typedef struct npbnn_sched_req {
    int asked;                 /* npbnn_chain_cfg.schedule */
    int D, K, M;               /* candidates per pass, iterations of the batch, widest proposal */
    int eval_wgs;              /* evaluating workgroups of an overlapped launch (held against NPBNN_SCHED_SPEC_PART_SLOTS) */
    int alone;                 /* no other chain's launches share the GPU with this batch */
    int plain;                 /* a plain run (no segments: an exchange run's kernels go between the passes) */
    int group;                 /* one chain of a group pass */
    int boundaries_only;       /* rows split over ranks, or the weight-streamed path: something runs between every pass and its step */
    int sync_failed;           /* a device-side wait of this context timed out once */
    int persist_option;        /* NPBNN_OPT_PERSISTENT */
    int has_spec_build;        /* this launch has a build with the speculative step */
    int own_slopes;            /* the batch carries trainable slopes */
    int prior_fits_spec;       /* uniform prior, or normal without per-weight scales */
    int no_spec_step;          /* NPBNN_NO_SPEC_STEP is set */
} npbnn_sched_req;

/* the schedule and what follows from it.  persist: one launch loops over the passes; sync: device flags order the passes (two launch
 * streams, or the persistent forms); spec: the launch's build with the speculative step, the next pass prepared ahead for every outcome */
typedef struct npbnn_sched_choice { int schedule, persist, overlap, sync, spec; } npbnn_sched_choice;

/* The schedule of the batch `r` describes on a context with history `h`.  What it changes in `h`: h->turn_batches[other][class] = 0 when
 * NPBNN_SCHED_AUTO sends the batch to the other persistent form as a probe, or finds that form's figure stale but out of reach. */
static inline npbnn_sched_choice npbnn_sched_choose(const npbnn_sched_req* r, npbnn_sched_hist* h) {
    const int D = r->D, K = r->K, M = r->M;
    /* (row shards: a gather between pass and step; weight-streamed path: the candidate image is patched between step and pass) */
    int schedule = r->group ? NPBNN_SCHED_OVERLAP : r->boundaries_only ? NPBNN_SCHED_SERIAL : r->asked;
    if (schedule != NPBNN_SCHED_SERIAL && schedule != NPBNN_SCHED_OVERLAP && schedule != NPBNN_SCHED_OVERLAP2 && schedule != NPBNN_SCHED_PERSIST &&
        schedule != NPBNN_SCHED_PERSIST_SERIAL) {
        /* overlapping the decision of a pass with the evaluation of the next pays as long as most passes reject everything */
        const double p_acc = h->accept_rate < 0 ? 0.0 : h->accept_rate;
        /* (measured, config-2 shapes, tools/stress_schedules.py 10000 1 2 4: up to 34 % of the proposals accepted - 71 % of the passes -
         * the overlapped forms lead, 48-63 k against 45-50 k it/s; config 4 at 46 % / 84 %: serial 18.8 k against 17.4-18.4 k) */
        schedule = (1.0 - pow(1.0 - p_acc, (double)D)) < 0.75 ? NPBNN_SCHED_OVERLAP : NPBNN_SCHED_SERIAL;
        /* Where overlapping pays and the chain has the GPU to itself, the persistent form of it: one launch whose workgroups loop
         * over the passes (no launch boundary between passes; a workgroup that is through with pass L starts pass L + 1 while
         * others still finish L).  Its device-side waits only need the launch's workgroups resident together - one per compute
         * unit, at most as many as there are - and are bounded: a time-out ends the batch with NPBNN_E_SYNC, state untouched, and
         * the context stays on kernel boundaries from then on.  (The two-stream form, NPBNN_SCHED_OVERLAP2, is never picked here:
         * it also needs the two streams on hardware queues of their own, which nothing promises.) */
        if (schedule == NPBNN_SCHED_OVERLAP && r->alone && r->plain && !r->sync_failed && r->persist_option)
            schedule = NPBNN_SCHED_PERSIST;
        /* A chain that moves: in the overlapped forms every pass that accepts something voids the pass in flight behind it (at 28 %
         * acceptance 63 % of the passes do), and on kernel boundaries a decision between two passes costs a step kernel and two
         * boundaries.  The persistent launch with the decision between the passes (NPBNN_SCHED_PERSIST_SERIAL) wastes no pass and
         * decides in a few microseconds: it leads where the predicted cost per decided pass says so (kSpecTurnExtraUs above).
         * (its step workgroup must keep pace with the evaluation: with proposals much wider than a few hundred weights it does not) */
        if (r->alone && r->plain && !r->sync_failed && r->persist_option && p_acc > 0.0 && !r->group &&
            !r->own_slopes && M <= kPersistSerialMaxWidth && r->has_spec_build && r->prior_fits_spec) {
            /* What decides is what a form was MEASURED to cost per iteration on this chain (it_us: a batch's time over its
             * iterations); the model - a decided pass costs (1 + a) turns overlapped, a turn + `extra` with the decision between the
             * passes - only prices the form that has not run yet from the one that has. */
            const double a = 1.0 - pow(1.0 - p_acc, (double)D);                      /* share of the passes that accept something */
            const double ipp = a / p_acc;                                    /* iterations a decided pass settles: 1 + (1-p) + ... + (1-p)^(D-1) */
            const double extra = kSpecTurnExtraUs + kSpecTurnExtraUsPerWeight * M;
            const int kc = K < kShortBatch ? 0 : 1;                          /* (a form's fixed cost per batch differs: short and long batches apart) */
            double c_over = h->it_us[0][kc], c_ser = h->it_us[1][kc];        /* us per iteration */
            if (c_over <= 0.0 && c_ser <= 0.0) c_over = kTurnUsGuess * (1.0 + a) / ipp;
            if (c_over <= 0.0) {
                const double t_over = c_ser * ipp - extra > 5.0 ? c_ser * ipp - extra : 5.0;
                c_over = t_over * (1.0 + a) / ipp;
            }
            if (c_ser <= 0.0) c_ser = (c_over * ipp / (1.0 + a) + extra) / ipp;
            /* (3 % in favour of the form the chain is on: no flipping on noise) */
            const int on_serial = h->last_schedule == NPBNN_SCHED_PERSIST_SERIAL;
            if (c_ser * (on_serial ? 0.97 : 1.03) < c_over) schedule = NPBNN_SCHED_PERSIST_SERIAL;
            /* a measured cost goes stale while the other form runs (the chain's acceptance rate moves, the box's clocks do): after
             * kTurnReprobeBatches batches on one form, one batch on the other - if it is within reach or was never run
             * (a form's first batch in a size class pays for the switch - other builds of the kernel, cold tables: it runs a second one
             * before its figure is held against the other's) */
            if (h->it_n[0][kc] == 1) schedule = NPBNN_SCHED_PERSIST;
            else if (h->it_n[1][kc] == 1) schedule = NPBNN_SCHED_PERSIST_SERIAL;
            const int other = schedule == NPBNN_SCHED_PERSIST_SERIAL ? 0 : 1;
            /* (a form never measured in this size class gets its batch after a handful on the other: the model is a prior, not a verdict -
             * it prices every accept of the overlapped form at a whole pass in vain, and such a pass is cut short) */
            const int since = h->turn_batches[other][kc];
            const int never = h->it_us[other][kc] <= 0.0;
            if (since >= (never ? kTurnFirstProbeBatches : kTurnReprobeBatches)) {
                const double ratio = other == 1 ? c_ser / c_over : c_over / c_ser;
                /* A form that has run: within a factor two, that is - its figure dates from when it last ran, the chain's acceptance rate has
                 * moved since, and with it both forms' costs; one batch in kTurnReprobeBatches costs a per cent at worst.  A form never
                 * run: when the model puts it within kFirstProbeWithin of the running one (at a few per cent acceptance the decision between
                 * the passes is predicted a fifth to a third dearer, and is: two batches on it would be two batches lost - a chain's first
                 * dispatches are where short runs are timed) - and whatever the model says after kTurnForcedProbeBatches, so that a wrong
                 * model cannot park a chain for good. */
                const int probe = never ? (ratio < kFirstProbeWithin || since >= kTurnForcedProbeBatches) : ratio < 2.0;
                if (probe || !never) h->turn_batches[other][kc] = 0;
                if (probe) schedule = other == 1 ? NPBNN_SCHED_PERSIST_SERIAL : NPBNN_SCHED_PERSIST;
            }
        }
    }
    if ((schedule == NPBNN_SCHED_OVERLAP2 || schedule == NPBNN_SCHED_PERSIST) && r->sync_failed) schedule = NPBNN_SCHED_OVERLAP;
    /* (asked for by name where it cannot run - no build with the speculative step for this launch, another prior, trainable slopes, a
     * shared GPU: the persistent overlapped form where that can, else kernel boundaries)
     * (the evaluating workgroups' tagged sums of that schedule sit in NPBNN_SCHED_SPEC_PART_SLOTS slots per value, and the step reads exactly
     * that many: a part with more compute units than slots - none today: 256 of each on gfx950 - stays on the overlapped form) */
    if (schedule == NPBNN_SCHED_PERSIST_SERIAL &&
        (r->eval_wgs > NPBNN_SCHED_SPEC_PART_SLOTS || r->sync_failed || !r->alone || !r->plain || r->group || !r->has_spec_build || r->own_slopes ||
         r->no_spec_step || !r->prior_fits_spec))
        schedule = (r->alone && r->plain && !r->sync_failed && !r->group) ? NPBNN_SCHED_PERSIST : NPBNN_SCHED_OVERLAP;
    /* the persistent form needs every workgroup of its launch resident at once: one per compute unit at most, the GPU to itself, and
     * a plain run (an exchange run's kernels go between the passes)
     * (its grid is at most one workgroup per compute unit: the evaluating workgroups are capped at n_cu - 1 by the caller, plus the step's) */
    if (schedule == NPBNN_SCHED_PERSIST && (!r->alone || !r->plain)) schedule = NPBNN_SCHED_OVERLAP;
    npbnn_sched_choice c;
    c.spec = schedule == NPBNN_SCHED_PERSIST_SERIAL;         /* (every condition was checked above) */
    c.persist = schedule == NPBNN_SCHED_PERSIST || c.spec;
    c.overlap = schedule == NPBNN_SCHED_OVERLAP || schedule == NPBNN_SCHED_OVERLAP2 || c.persist;
    c.sync = (schedule == NPBNN_SCHED_OVERLAP2 && r->alone) || c.persist;     /* (several chains on one GPU: one stream each) */
    if (schedule == NPBNN_SCHED_OVERLAP2 && !c.sync) schedule = NPBNN_SCHED_OVERLAP;
    c.schedule = schedule;
    return c;
}

/* after every batch, whatever ran it: `k_take` iterations handed back, decided in `n_turns` launch turns (passes, decided or void) */
static inline void npbnn_sched_record_outcome(npbnn_sched_hist* h, int schedule, int k_take, int n_turns, int n_accepted) {
    if (n_turns > 0 && k_take > 0) h->its_per_pass = (double)k_take / n_turns;
    h->last_schedule = schedule;
    if (k_take > 0) h->accept_rate = (double)n_accepted / k_take;
}

/* after a plain batch of K iterations that took `batch_us` from its first launch to its results, in `n_rounds` rounds of `n_turns`
 * turns in all: what a turn of this form takes here, and what an iteration cost on it (what NPBNN_SCHED_AUTO compares) */
static inline void npbnn_sched_record_timing(npbnn_sched_hist* h, int schedule, int persist, int K, int n_rounds, int n_turns, double batch_us) {
    if (!(persist && n_rounds == 1 && n_turns >= 8)) return;
    const int form = schedule == NPBNN_SCHED_PERSIST_SERIAL ? 1 : 0, kc = K < kShortBatch ? 0 : 1;
    double* t = &h->turn_us[form];
    double now_us = batch_us / n_turns;
    /* one stalled call (the host descheduled, a collector pause: 80 ms were seen) must not price a form out for good - the form
     * that lost is not run again, so nothing would ever correct its estimate: a sample counts for at most 1.25 x the estimate */
    if (*t > 0.0 && now_us > 1.25 * *t) now_us = 1.25 * *t;
    *t = *t > 0.0 ? 0.75 * *t + 0.25 * now_us : now_us;
    double* c = &h->it_us[form][kc];                   /* ... and what an iteration cost on it, in batches of this size class */
    double it_now = batch_us / K;
    int* n_seen = &h->it_n[form][kc];
    if (*n_seen == 1) *c = it_now < *c ? it_now : *c;  /* (the better of a form's first two batches) */
    else {
        if (*c > 0.0 && it_now > 1.25 * *c) it_now = 1.25 * *c;
        *c = *c > 0.0 ? 0.75 * *c + 0.25 * it_now : it_now;
    }
    if (*n_seen < 1000) ++*n_seen;
    h->turn_batches[form][kc] = 0;
    h->turn_batches[1 - form][kc] += 1;
}

/* passes to launch for `rem` iterations: a pass decides between 1 and D of them; what the previous batch's average says is
 * needed plus a margin (passes launched after the last iteration return at once) */
static inline int npbnn_sched_passes(int rem, int D, int persist, int overlap, double its_per_pass, double slack) {
    int n = (rem + D - 1) / D;
    /* the persistent launch ends by itself at the chain's terminal pass, so a generous bound costs nothing - and a second round
     * (results back, look, launch again) costs a host round trip: the worst case, every iteration accepted (one iteration per
     * pass and a void pass after each) */
    if (persist) return 2 * rem + 4;
    if (its_per_pass >= 1.0) {
        const int est = (int)ceil(slack * (double)rem / its_per_pass);
        if (est > n) n = est;
        /* a launch past the end of the batch returns at once (a few microseconds); coming back short costs a host round trip and a
         * second round: lean towards the former */
        n += 3 + n / 8;
    }
    if (overlap) n += 1;                     /* the last pass is decided by the launch after it */
    return n;
}

/* the same for a segment of an exchange run, where falling short is expensive (no second round): with no history, the
 * worst case (every iteration accepted: one iteration per pass, and in the overlapped schedule a void pass after each) */
static inline int npbnn_sched_passes_segment(int seg_len, int D, int overlap, double its_per_pass, double slack) {
    double est = its_per_pass >= 1.0 ? (double)seg_len / its_per_pass : (double)seg_len * (overlap ? 2.0 : 1.0);
    const double least = (double)((seg_len + D - 1) / D);
    if (est < least) est = least;
    return (int)ceil(slack * est) + 2 + (overlap ? 1 : 0);
}

/* launches of a group pass for `rem` iterations of its slowest chain: a launch decides at most one iteration per chain and loses one
 * to every accept (the pass in flight is void) - `acc`: the highest of the chains' last acceptance rates */
static inline int npbnn_sched_passes_group(int rem, double acc) {
    return (int)ceil((double)rem * (1.0 + acc) * 1.05) + 3;
}

#endif
