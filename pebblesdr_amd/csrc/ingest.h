// ingest.h -- host ingest: the pinned double buffer (the library owns the pinned host buffers; the producer side of
// plugins/HackRFDevice/hackrfdevice.cpp:533-566 writes into them instead of into its own ring).  Two slots per handle: the host fills
// one while the call that reads the other's device twin is still queued.  Shared by Receiver and the stream bank (cores.hip).
#pragma once
#include "common.h"
#include "devmem.h"

namespace pg {

struct IngestSlot {
    PinnedBuf<unsigned char> h;           // pinned host buffer ...
    DevBuf<unsigned char> d;              // ... and its device twin
    size_t cap = 0, submitted = 0;
    hipEvent_t uploaded = nullptr, done_main = nullptr, done_chain = nullptr;
    bool in_flight = false;               // a call that reads the device twin has been queued and not waited for
};

struct IngestRing {
    IngestSlot slot[2];
    hipStream_t copy_stream = nullptr;
    // acquire: waits for the call that last read the slot, (re)allocates, hands out the pinned buffer
    int acquire(int device, uint32_t s, uint64_t bytes, void **host_ptr);
    // submit: queues the upload of the first `bytes` on the copy stream
    int submit(int device, uint32_t s, uint64_t bytes);
    // the checks of a process_ingested call, before anything is queued: `pairs` IQ pairs of `fmt` must fit what was submitted
    int check(uint32_t s, int fmt, uint64_t pairs, uint64_t n_for_message, IngestSlot **g);
    // both of a call's streams read the raw samples: they wait for the upload, and the slot is free again when both are past the call
    int wait_upload(IngestSlot &g, hipStream_t main, hipStream_t chain);
    int mark_in_flight(IngestSlot &g, hipStream_t main, hipStream_t chain);
    // A ring fed from a pinned host buffer that somebody else owns (the multibank's slots, shared by every shard: multibank.hip).  Such a
    // ring has device twins only (slot.h stays null) and is never handed to acquire / submit:
    //   wait_free   -- blocks until the last call that read the slot's twin, and any upload still queued, is over
    //   submit_from -- queues the upload of `bytes` from h_src (pinned, readable by this device) into the twin (grown on demand)
    int wait_free(uint32_t s);
    int submit_from(int device, uint32_t s, const void *h_src, uint64_t bytes);
    void release();  // (the owner has synchronised its own streams)
};

}  // namespace pg
