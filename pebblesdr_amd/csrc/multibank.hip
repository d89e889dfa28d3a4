// multibank.hip -- pebblegpu_multibank_*: one process, one consumer thread, a bank's channels sharded across devices.
// No kernel lives here: a shard is an ordinary pebblegpu_receiver and every sample goes through the kernels a single-device bank runs.
// This file is the layer above the shards: the partition, the fan-out of the host's samples (one host-to-device copy per shard out of
// a pinned buffer every device can read; no peer copies), and one persistent host worker per shard, so that G shards are queued in
// the time one takes (a bank call costs the host about as long to queue as the GPU needs to run it).
#include <condition_variable>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include "receiver.h"

using pg::fail;

namespace {

enum JobKind { JOB_NONE = 0, JOB_PROCESS, JOB_PROCESS_RAW, JOB_WAIT_SLOT, JOB_UPLOAD, JOB_PROCESS_UPLOADED, JOB_SYNC };

struct Job {
    JobKind kind = JOB_NONE;
    const void *const *ptrs = nullptr;  // PROCESS / PROCESS_RAW: the caller's array, entry g for shard g
    uint64_t n = 0;
    int fmt = 0, order = 0;
    double gain = 1.0;
    uint32_t slot = 0;
};

struct HostSlot {
    pg::PortableBuf<unsigned char> h;  // pinned, portable: every device reads it
    uint64_t cap = 0;
    uint64_t submitted = 0;  // bytes of the last submit (0: nothing to process)
    bool in_flight = false;  // a process_ingested call has been queued on it and the slot has not been acquired since
    bool touched = false;    // a shard may still have an upload or a call on it
};

}  // namespace

struct pebblegpu_multibank {
    pebblegpu_config cfg{};
    uint32_t flags = 0, G = 0;
    bool shared = true;
    uint32_t first[PEBBLEGPU_MULTIBANK_MAX_SHARDS] = {}, count[PEBBLEGPU_MULTIBANK_MAX_SHARDS] = {};
    int32_t device[PEBBLEGPU_MULTIBANK_MAX_SHARDS] = {};
    pebblegpu_receiver *shard[PEBBLEGPU_MULTIBANK_MAX_SHARDS] = {};
    uint64_t superframe = 0;
    uint32_t max_sf = 1;
    HostSlot slot[2];
    // a shard failed or refused after others had queued: the shards' streams no longer agree (like Receiver::failed_)
    bool failed = false;
    std::string failed_text;

    // the workers: the caller posts one job to all of them and waits until every one has QUEUED its part
    std::thread worker[PEBBLEGPU_MULTIBANK_MAX_SHARDS];
    uint32_t n_workers = 0;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    uint64_t job_seq = 0;
    Job job;
    uint32_t pending = 0;
    bool stop = false;
    int rc[PEBBLEGPU_MULTIBANK_MAX_SHARDS] = {};
    std::string err[PEBBLEGPU_MULTIBANK_MAX_SHARDS];

    int run_job(uint32_t g, const Job &j);
    void work(uint32_t g);
    int post(const Job &j);
    void stop_workers();
};

int pebblegpu_multibank::run_job(uint32_t g, const Job &j)
{
    pg::Receiver &rx = shard[g]->rx;
    switch (j.kind) {
    case JOB_PROCESS: return rx.process((const float2 *)j.ptrs[g], j.n, rx.bins != 0, true);
    case JOB_PROCESS_RAW: return rx.process_raw(j.fmt, j.order, j.gain, j.ptrs[g], j.n);
    case JOB_WAIT_SLOT: return rx.ingest_wait(j.slot);
    case JOB_UPLOAD: {
        // a shared stream: every shard gets all of it; independent streams: the shard's rows of the [stream][time] buffer
        const HostSlot &s = slot[j.slot];
        if (shared) return rx.ingest_upload(j.slot, s.h, j.n);
        const uint64_t row = j.n / cfg.n_channels;
        return rx.ingest_upload(j.slot, (const char *)s.h.get() + row * first[g], row * count[g]);
    }
    case JOB_PROCESS_UPLOADED: return rx.process_uploaded(j.slot, j.fmt, j.order, j.gain, j.n);
    case JOB_SYNC: return rx.sync();
    default: return 0;
    }
}

void pebblegpu_multibank::work(uint32_t g)
{
    (void)hipSetDevice(device[g]);  // once: everything this thread queues is for this shard's device
    uint64_t seen = 0;
    for (;;) {
        Job j;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_job.wait(lk, [&] { return stop || job_seq != seen; });
            if (stop) return;
            seen = job_seq;
            j = job;
        }
        const int r = run_job(g, j);
        std::string text;
        if (r) text = pg::last_error();  // thread-local: carried to the caller by hand
        {
            std::lock_guard<std::mutex> lk(mu);
            rc[g] = r;
            err[g].swap(text);
            if (--pending == 0) cv_done.notify_one();
        }
    }
}

// returns when every worker has queued its part; the first failing shard's code, its text re-raised on the calling thread
int pebblegpu_multibank::post(const Job &j)
{
    std::unique_lock<std::mutex> lk(mu);
    job = j;
    pending = G;
    job_seq++;
    cv_job.notify_all();
    cv_done.wait(lk, [&] { return pending == 0; });
    for (uint32_t g = 0; g < G; g++)
        if (rc[g]) return fail(rc[g], "shard %u (device %d): %s", g, device[g], err[g].c_str());
    return 0;
}

void pebblegpu_multibank::stop_workers()
{
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = true;
    }
    cv_job.notify_all();
    for (uint32_t g = 0; g < n_workers; g++)
        if (worker[g].joinable()) worker[g].join();
    n_workers = 0;
}

static int plan_checked(uint32_t C, uint32_t G, uint32_t *first, uint32_t *count)
{
    if (!first || !count) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (G == 0 || G > PEBBLEGPU_MULTIBANK_MAX_SHARDS) return fail(PEBBLEGPU_E_INVALID, "n_shards must be 1..%d", PEBBLEGPU_MULTIBANK_MAX_SHARDS);
    if (C < G) return fail(PEBBLEGPU_E_INVALID, "%u channels do not fill %u shards", C, G);
    for (uint32_t g = 0; g < G; g++) {
        const uint32_t a = (uint32_t)((uint64_t)g * C / G), b = (uint32_t)((uint64_t)(g + 1) * C / G);
        first[g] = a;
        count[g] = b - a;
    }
    return 0;
}

// the checks every process call makes once, before any worker is asked: a refusal leaves every shard untouched
static int call_checks(pebblegpu_multibank *mb, uint64_t n)
{
    if (mb->failed) return fail(PEBBLEGPU_E_HIP, "an earlier call on this multibank failed on one shard after others had queued (%s): "
                                                 "its shards no longer agree, destroy it", mb->failed_text.c_str());
    if (n == 0) return fail(PEBBLEGPU_E_INVALID, "zero samples");
    if (n % mb->superframe != 0 || n / mb->superframe > mb->max_sf)
        return fail(PEBBLEGPU_E_SIZE, "n_samples %llu is not 1..%u super-frames of %llu", (unsigned long long)n, mb->max_sf, (unsigned long long)mb->superframe);
    return 0;
}

static int raw_checks(int format, int iq_order)
{
    if (format < 0 || format > PEBBLEGPU_IQ_WAV16 || iq_order < 0 || iq_order > 3)
        return fail(PEBBLEGPU_E_INVALID, "unknown sample format %d / IQ order %d", format, iq_order);
    return 0;
}

// a process job that came back with an error: some shards have queued the call and some have not
static int process_posted(pebblegpu_multibank *mb, const Job &j)
{
    const int rc = mb->post(j);
    if (rc) {
        mb->failed = true;
        mb->failed_text = pg::last_error();
    }
    return rc;
}

extern "C" {

int pebblegpu_multibank_plan(uint32_t n_channels, uint32_t n_shards, uint32_t *first, uint32_t *count)
{
    return plan_checked(n_channels, n_shards, first, count);
}

int pebblegpu_multibank_create(const pebblegpu_config *cfg, const int32_t *device_ids, uint32_t n_shards, uint32_t flags, pebblegpu_multibank **out)
{
    // arguments first, before any device is touched
    if (!cfg || !device_ids || !out) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (cfg->struct_size != sizeof(pebblegpu_config)) return fail(PEBBLEGPU_E_INVALID, "pebblegpu_config size mismatch (ABI %d)", PEBBLEGPU_ABI_VERSION);
    if (flags & ~(uint32_t)PEBBLEGPU_MULTIBANK_SPECTRUM_SHARD0) return fail(PEBBLEGPU_E_INVALID, "unknown flag bits 0x%x", flags);
    uint32_t first[PEBBLEGPU_MULTIBANK_MAX_SHARDS], count[PEBBLEGPU_MULTIBANK_MAX_SHARDS];
    if (int rc = plan_checked(cfg->n_channels, n_shards, first, count)) return rc;
    const int n_dev = pebblegpu_device_count();
    if (n_dev <= 0) return fail(PEBBLEGPU_E_NO_DEVICE, "no HIP device visible: libpebblegpu has no CPU path");
    for (uint32_t g = 0; g < n_shards; g++)
        if (device_ids[g] < 0 || device_ids[g] >= n_dev)
            return fail(PEBBLEGPU_E_INVALID, "shard %u: device %d out of range (0..%d)", g, device_ids[g], n_dev - 1);
    pebblegpu_multibank *mb = new (std::nothrow) pebblegpu_multibank();
    if (!mb) return fail(PEBBLEGPU_E_INVALID, "out of host memory");
    mb->cfg = *cfg;
    mb->flags = flags;
    mb->G = n_shards;
    mb->shared = cfg->shared_input != 0;
    for (uint32_t g = 0; g < n_shards; g++) {
        mb->first[g] = first[g];
        mb->count[g] = count[g];
        mb->device[g] = device_ids[g];
        pebblegpu_config c = *cfg;
        c.device = device_ids[g];
        c.n_channels = count[g];
        if (g > 0 && (flags & PEBBLEGPU_MULTIBANK_SPECTRUM_SHARD0)) c.spectrum_bins = c.hires_bins = 0;
        if (int rc = pebblegpu_receiver_create(&c, &mb->shard[g])) {
            const std::string text = pg::last_error();
            for (uint32_t k = 0; k < g; k++) (void)pebblegpu_receiver_destroy(mb->shard[k]);
            delete mb;
            return fail(rc, "shard %u (device %d, %u channels): %s", g, device_ids[g], count[g], text.c_str());
        }
    }
    mb->superframe = mb->shard[0]->rx.superframe;  // the chain's geometry does not depend on the channel count
    mb->max_sf = mb->shard[0]->rx.max_sf;
    for (uint32_t g = 0; g < n_shards; g++) {
        mb->worker[g] = std::thread(&pebblegpu_multibank::work, mb, g);
        mb->n_workers = g + 1;
    }
    *out = mb;
    return 0;
}

int pebblegpu_multibank_destroy(pebblegpu_multibank *mb)
{
    if (!mb) return 0;
    Job j;
    j.kind = JOB_SYNC;
    (void)mb->post(j);  // every shard's queued work first,
    mb->stop_workers();  // then the workers,
    for (uint32_t g = 0; g < mb->G; g++) (void)pebblegpu_receiver_destroy(mb->shard[g]);  // then the shards (and their device twins)
    delete mb;  // (and the pinned slots)
    return 0;
}

int pebblegpu_multibank_shards(const pebblegpu_multibank *mb, uint32_t *n_shards)
{
    if (!mb || !n_shards) return fail(PEBBLEGPU_E_INVALID, "null argument");
    *n_shards = mb->G;
    return 0;
}

int pebblegpu_multibank_shard(pebblegpu_multibank *mb, uint32_t g, pebblegpu_receiver **rx, int32_t *device, uint32_t *first_channel, uint32_t *n_channels)
{
    if (!mb) return fail(PEBBLEGPU_E_INVALID, "null handle");
    if (g >= mb->G) return fail(PEBBLEGPU_E_INVALID, "shard %u out of range (%u shards)", g, mb->G);
    if (rx) *rx = mb->shard[g];
    if (device) *device = mb->device[g];
    if (first_channel) *first_channel = mb->first[g];
    if (n_channels) *n_channels = mb->count[g];
    return 0;
}

int pebblegpu_multibank_locate(const pebblegpu_multibank *mb, uint32_t channel, uint32_t *shard, uint32_t *local_channel)
{
    if (!mb) return fail(PEBBLEGPU_E_INVALID, "null handle");
    if (channel >= mb->cfg.n_channels) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range (%u channels)", channel, mb->cfg.n_channels);
    uint32_t g = 0;
    while (channel >= mb->first[g] + mb->count[g]) g++;
    if (shard) *shard = g;
    if (local_channel) *local_channel = channel - mb->first[g];
    return 0;
}

int pebblegpu_multibank_process(pebblegpu_multibank *mb, const void *const *d_iq, uint64_t n_samples)
{
    if (!mb || !d_iq) return fail(PEBBLEGPU_E_INVALID, "null argument");
    for (uint32_t g = 0; g < mb->G; g++)
        if (!d_iq[g]) return fail(PEBBLEGPU_E_INVALID, "null input for shard %u", g);
    if (int rc = call_checks(mb, n_samples)) return rc;
    Job j;
    j.kind = JOB_PROCESS;
    j.ptrs = d_iq;
    j.n = n_samples;
    return process_posted(mb, j);
}

int pebblegpu_multibank_process_raw(pebblegpu_multibank *mb, int format, int iq_order, double gain, const void *const *d_raw, uint64_t n_samples)
{
    if (!mb || !d_raw) return fail(PEBBLEGPU_E_INVALID, "null argument");
    for (uint32_t g = 0; g < mb->G; g++)
        if (!d_raw[g]) return fail(PEBBLEGPU_E_INVALID, "null input for shard %u", g);
    // (the receivers refuse a misaligned pointer themselves; here, before any worker is asked, the refusal leaves every shard untouched)
    for (uint32_t g = 0; g < mb->G; g++)
        if (reinterpret_cast<uintptr_t>(d_raw[g]) % PEBBLEGPU_RAW_ALIGN)
            return fail(PEBBLEGPU_E_INVALID, "d_raw of shard %u must be aligned to %d bytes", g, PEBBLEGPU_RAW_ALIGN);
    if (int rc = raw_checks(format, iq_order)) return rc;
    if (int rc = call_checks(mb, n_samples)) return rc;
    Job j;
    j.kind = JOB_PROCESS_RAW;
    j.ptrs = d_raw;
    j.n = n_samples;
    j.fmt = format;
    j.order = iq_order;
    j.gain = gain;
    return process_posted(mb, j);
}

int pebblegpu_multibank_ingest_acquire(pebblegpu_multibank *mb, uint32_t slot, uint64_t bytes, void **host_ptr)
{
    if (!mb || !host_ptr) return fail(PEBBLEGPU_E_INVALID, "null argument");
    if (slot > 1 || bytes == 0) return fail(PEBBLEGPU_E_INVALID, "ingest slot is 0 or 1, bytes > 0");
    HostSlot &s = mb->slot[slot];
    if (s.touched) {  // every shard's last call that read its twin of this slot (and any upload nobody processed) must be over
        Job j;
        j.kind = JOB_WAIT_SLOT;
        j.slot = slot;
        if (int rc = mb->post(j)) return rc;
        s.touched = s.in_flight = false;
    }
    s.submitted = 0;
    if (s.cap < bytes) {
        PG_HIP(hipSetDevice(mb->device[0]));
        s.cap = 0;
        PG_TRY(s.h.alloc(bytes));
        s.cap = bytes;
    }
    *host_ptr = s.h;
    return 0;
}

int pebblegpu_multibank_ingest_submit(pebblegpu_multibank *mb, uint32_t slot, uint64_t bytes)
{
    if (!mb) return fail(PEBBLEGPU_E_INVALID, "null handle");
    if (slot > 1) return fail(PEBBLEGPU_E_INVALID, "ingest slot is 0 or 1");
    HostSlot &s = mb->slot[slot];
    if (!s.h || bytes == 0 || bytes > s.cap) return fail(PEBBLEGPU_E_SIZE, "%llu bytes do not fit the slot acquired (%llu)", (unsigned long long)bytes, (unsigned long long)s.cap);
    if (s.in_flight || s.submitted) return fail(PEBBLEGPU_E_INVALID, "the slot has been submitted already: acquire it again first");
    if (!mb->shared && bytes % mb->cfg.n_channels != 0)
        return fail(PEBBLEGPU_E_SIZE, "%llu bytes are not %u equal rows ([stream][time])", (unsigned long long)bytes, mb->cfg.n_channels);
    Job j;
    j.kind = JOB_UPLOAD;
    j.slot = slot;
    j.n = bytes;
    s.touched = true;
    if (int rc = mb->post(j)) return rc;  // (nothing of the chain has been queued: the shards still agree; the slot must be acquired again)
    s.submitted = bytes;
    return 0;
}

int pebblegpu_multibank_process_ingested(pebblegpu_multibank *mb, uint32_t slot, int format, int iq_order, double gain, uint64_t n_samples)
{
    if (!mb) return fail(PEBBLEGPU_E_INVALID, "null handle");
    if (slot > 1) return fail(PEBBLEGPU_E_INVALID, "ingest slot is 0 or 1");
    if (int rc = raw_checks(format, iq_order)) return rc;
    if (int rc = call_checks(mb, n_samples)) return rc;
    HostSlot &s = mb->slot[slot];
    const uint64_t row = n_samples * pg::kRawPairBytes[format];
    if (s.in_flight) return fail(PEBBLEGPU_E_INVALID, "the slot's samples have been processed: acquire, fill and submit it again first");
    if (!s.submitted) return fail(PEBBLEGPU_E_SIZE, "nothing has been submitted to slot %u", slot);
    if (mb->shared ? row > s.submitted : row * mb->cfg.n_channels != s.submitted)
        return fail(PEBBLEGPU_E_SIZE, "the slot holds %llu submitted bytes; %llu samples of this format per stream need %s%llu",
                    (unsigned long long)s.submitted, (unsigned long long)n_samples, mb->shared ? "" : "exactly ",
                    (unsigned long long)(mb->shared ? row : row * mb->cfg.n_channels));
    Job j;
    j.kind = JOB_PROCESS_UPLOADED;
    j.slot = slot;
    j.n = n_samples;
    j.fmt = format;
    j.order = iq_order;
    j.gain = gain;
    s.in_flight = true;
    return process_posted(mb, j);
}

int pebblegpu_multibank_synchronize(pebblegpu_multibank *mb)
{
    if (!mb) return fail(PEBBLEGPU_E_INVALID, "null handle");
    Job j;
    j.kind = JOB_SYNC;
    return mb->post(j);
}

int pebblegpu_multibank_last_ms(const pebblegpu_multibank *mb, float *max_over_shards)
{
    if (!mb || !max_over_shards) return fail(PEBBLEGPU_E_INVALID, "null argument");
    float worst = 0.f;
    for (uint32_t g = 0; g < mb->G; g++) {
        float ms = 0.f;
        PG_HIP(hipSetDevice(mb->device[g]));
        if (int rc = pebblegpu_receiver_last_ms(mb->shard[g], 0, &ms)) return rc;
        if (ms > worst) worst = ms;
    }
    *max_over_shards = worst;
    return 0;
}

}  // extern "C"
