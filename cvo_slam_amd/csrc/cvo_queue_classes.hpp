// Queue classes of the library's own batch streams: the pure bookkeeping, free of HIP so that a host test can compile it
// (tests/test_queue_classes_host.py).  The HIP runtime maps the streams of ONE priority onto at most Q hardware queues
// (hw_queue_count in cvo_capi.hip) and keeps that limit per priority, so streams dealt over two priorities can have 2 Q
// hardware queues between them.  Class 0 is the normal priority, class 1 the second priority the dealer uses (the least
// one; DESIGN.md section 4.1, "Queue classes").  The greatest priority is never a class: it belongs to the stage streams.
#pragma once

namespace cvo_qc {

constexpr int CLASSES = 2;

// The class of an engine about to be made.  live[c]: library-made engine streams of this device alive in class c (this one
// not counted yet).  dealt: the engine's stream may be dealt (a batch object of the public API); every other engine is
// class 0 -- and is counted there all the same.  second_class: the device has a priority level for class 1 and the dealer
// is on.  Class 0 while it has fewer than Q streams, then class 1 while it has fewer than Q, then whichever has fewer
// (class 0 on a tie).
inline int choose_class(const int live[CLASSES], int Q, bool dealt, bool second_class) {
    if (!dealt || !second_class) return 0;
    if (live[0] < Q) return 0;
    if (live[1] < Q) return 1;
    return live[1] < live[0] ? 1 : 0;
}

// How much of the device an align launch about to be submitted on an engine of class `mine` can count on.  inflight[c]:
// align launches of the library in flight on the device's OTHER engines of class c.  Every class runs at most Q launches
// side by side, each on its own hardware queue, so concurrent = sum over c of min(Q, inflight[c] + (c == mine)); the
// launch waits behind another one of its own class when that class has no queue left: deferred = inflight[mine] >= Q.
// With one class in use these are min(Q, inflight + 1) and inflight >= Q.
inline void launch_share(const int inflight[CLASSES], int mine, int Q, int* concurrent, bool* deferred) {
    int sum = 0;
    for (int c = 0; c < CLASSES; ++c) {
        const int k = inflight[c] + (c == mine ? 1 : 0);
        sum += k < Q ? k : Q;
    }
    *concurrent = sum;
    *deferred = inflight[mine] >= Q;
}

}  // namespace cvo_qc
