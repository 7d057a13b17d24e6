// kzg_handle.inc -- what the handles of the KZG drivers share (zkp_kzg_opener in g1_ntt_host.inc, zkp_kzg_recoverer in
// kzg_recover_host.inc, zkp_kzg_cell_verifier in kzg_cells_host.inc): who owns a handle's workspace and drains the device before it
// goes, the pinned buffer a call stages its host-made tables in, the refusal before anything is allocated, the slot's staging
// buffer of the host-pointer entries and the table of a root's powers (fr_pow2.hpp).  Included by api.hip before the three drivers.

namespace {

// What every handle holds; the opaque structs derive from it and add their own.  `work` (the sizes of the handle's plan header;
// entries of a slot are serialised, so one call uses it at a time) is destroyed after the derived members, not among them as it
// once was: immaterial, since handle_destroy has drained the device before any member goes.
struct KzgHandle {
    unsigned log_n = 0, log_l = 0;
    int slot = 0, device = 0;
    DevBuf work;
};

// The one teardown.  The members' destructors neither synchronise nor switch device (dev_res.hpp), so the handle's device is made
// current and drained here first; the caller keeps its own.
template <class H>
void handle_destroy(H* h) {
    if (!h) return;
    DeviceRestore restore;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();  // a call may still be running on the caller's stream
    delete h;
}

// A handle of the slot the caller has entered, torn down as above unless the creation releases it to its caller; null: no memory
template <class H>
std::unique_ptr<H, void (*)(H*)> handle_new(unsigned log_n, unsigned log_l) {
    std::unique_ptr<H, void (*)(H*)> h(new (std::nothrow) H(), handle_destroy<H>);
    if (!h) return h;
    h->log_n = log_n;
    h->log_l = log_l;
    h->slot = ctx().slot;
    h->device = ctx().device;
    return h;
}

// The pinned buffer a call fills with what the host makes for it (index lists, masks, tables) and copies from on the call's stream.
// The copy is asynchronous, so the next call may overwrite the buffer only when the event recorded behind that copy has passed:
// acquire() before writing, sent() behind the last copy.  That event is all a *_dev entry ever waits for, and neither call
// allocates: make(), at creation, has made the buffer and the event.
struct HostStage {
    PinnedBuf buf;
    Event copied;
    bool stage_pending = false;
    int make(size_t bytes) { return buf.grow(bytes) == hipSuccess ? copied.ensure(hipEventDisableTiming) : ZKP_E_NOMEM; }
    int acquire() {
        if (stage_pending) HIPCHK(hipEventSynchronize(copied));
        stage_pending = false;
        return ZKP_OK;
    }
    int sent(hipStream_t st) {
        HIPCHK(hipEventRecord(copied, st));
        stage_pending = true;
        return ZKP_OK;
    }
};

// Refuse before allocating: ZKP_E_NOMEM with `head` + ", F of T bytes free on the device" when `total` device bytes exceed the
// budget of `knob` (KNOB_COUNT: none; else its name and value end the message) or the free memory plus `spare` (bytes the growth
// frees first).  grow() then allocates and says whether all of it succeeded; a failure ends in the same message, and the owner of
// the buffers releases what it got.
template <class Grow>
int reserve_or_refuse(size_t total, Knob knob, const std::string& head, Grow&& grow, size_t spare = 0) {
    const size_t budget = knob == KNOB_COUNT ? SIZE_MAX : (size_t)knob_int(knob);
    const DevFree mem;
    if (total <= budget && (!mem.total_b || total <= mem.free_b + spare) && grow()) return ZKP_OK;
    (void)hipGetLastError();
    return mem.refuse(head, knob == KNOB_COUNT ? "" : std::string(", ") + kKnobs[knob].name + " " + std::to_string(budget));
}

// The slot's staging buffer, where a host-pointer entry keeps the device copies of its arguments, grown to `need` bytes (a failed
// growth leaves it released)
int slot_workspace(size_t need, const char* what, void** out) {
    DevBuf& tmp = ctx().tmp;
    if (need > tmp.cap) {
        const int rc = reserve_or_refuse(need, KNOB_COUNT, std::string(what) + ": the workspace of " + std::to_string(need) + " bytes does not fit",
                                         [&] { return tmp.grow(need) == hipSuccess; }, tmp.cap);
        if (rc != ZKP_OK) tmp.release();
        ZCHK(rc);
    }
    *out = tmp.p;
    return ZKP_OK;
}

FrPow2 fr_pow2_table(HFr x) {
    FrPow2 t;
    for (unsigned b = 0; b < FR_POW2_BITS; b++, x = x.sqr()) t.p[b] = HostField<Fr>::dev(x);
    return t;
}

}  // namespace
