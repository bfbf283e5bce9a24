/*
 * nstack.c — socket layer of the stack (host C) over librxgpu.
 *
 * Control blocks, lists and socket calls follow the reference
 * (common.c:262-666, udp.h:10-44, tcp.h:29-84); the receive path is a GPU
 * burst (rxg_process_mbufs) followed by UDP delivery with the reference's
 * offload semantics (udp.c:25-52).  See include/nstack.h for the deliberate
 * differences.
 */
#define _GNU_SOURCE
#include "../../include/nstack.h"

#include <errno.h>
#include <netinet/in.h>
#include <pthread.h>
#include <sched.h>
#include <stdatomic.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define D_DEFAULT_FD_NUM 3   /* common.h:33 */
#define D_MAX_FD_COUNT 1024  /* common.h:34 */
#define D_RING_SIZE 1024     /* common.h:29 */
#define D_TCP_INITIAL_WINDOW 14600
#define D_TCP_MAX_SEQ 0xffffffffu /* common.h:40 */
#define TCP_FIN 0x01
#define TCP_SYN 0x02
#define TCP_PSH 0x08
#define TCP_ACK 0x10

enum {
    TCP_STATUS_CLOSED = 0,
    TCP_STATUS_LISTEN,
    TCP_STATUS_SYN_RCVD,
    TCP_STATUS_SYN_SENT,
    TCP_STATUS_ESTABLISHED,
    TCP_STATUS_FIN_WAIT_1,
    TCP_STATUS_FIN_WAIT_2,
    TCP_STATUS_CLOSING,
    TCP_STATUS_TIME_WAIT,
    TCP_STATUS_CLOSE_WAIT,
    TCP_STATUS_LAST_ACK
}; /* tcp.h:10-26 */

/* ---- rings (stand-in for rte_ring; guarded by the owner's mutex) --------
 * The slot entries and head are stored with relaxed atomic stores: drain_all
 * reads the head slot of the next block's ring without its mutex, as a
 * prefetch hint (a value possibly stale, never dereferenced), and those
 * reads are then no data race. */
struct nring {
    void **slot;
    uint32_t cap, head, count;
};

/* rings live inside their control block (one line fewer for a reader to
 * fetch); only the slot array is allocated */
static struct nring *ring_init(struct nring *r, uint32_t cap) {
    r->slot = calloc(cap, sizeof(void *));
    if (!r->slot) return NULL;
    r->cap = cap;
    r->head = r->count = 0;
    return r;
}
static void ring_free(struct nring *r) {
    if (r) {
        free(r->slot);
        r->slot = NULL;
    }
}
static int ring_enqueue(struct nring *r, void *p) {
    if (r->count == r->cap) return -ENOBUFS;
    __atomic_store_n(&r->slot[(r->head + r->count) % r->cap], p, __ATOMIC_RELAXED);
    r->count++;
    return 0;
}
static int ring_peek(struct nring *r, void **p) {
    if (!r->count) return -ENOENT;
    *p = r->slot[r->head];
    return 0;
}
static int ring_peek_at(struct nring *r, uint32_t k, void **p) {
    if (k >= r->count) return -ENOENT;
    *p = r->slot[(r->head + k) % r->cap];
    return 0;
}
static int ring_dequeue(struct nring *r, void **p) {
    if (!r->count) return -ENOENT;
    *p = r->slot[r->head];
    __atomic_store_n(&r->head, (r->head + 1) % r->cap, __ATOMIC_RELAXED);
    r->count--;
    return 0;
}

/* ---- control blocks (udp.h:10-44, tcp.h:29-84) ------------------------- */
struct localhost {
    int fd;
    uint32_t localip;
    unsigned char localmac[6];
    uint16_t localport;
    unsigned char protocol; /* (@16 in both block kinds: get_hostinfo_fromfd's cast) */
    struct nring *sndbuf, *rcvbuf;
    uint32_t flow_id; /* stable id in the GPU flow tables (verdict flow_id) */
    uint32_t queued;  /* datagrams in rcvbuf (a batch item holds several) */
    /* what a reader touches, together: the lock, the receive ring, the state */
    pthread_mutex_t mutex;
    struct nring rcv_r;
    atomic_int ref;   /* the lists' reference + one per reader (cb_get / udp_put) */
    int dead;         /* unlinked (nclose): readers return, the last put frees */
    struct nring snd_r;
    struct localhost *prev, *next;
    pthread_cond_t cond;
};

struct dgram_batch;
struct offload {
    uint32_t sip, dip;
    uint16_t sport, dport;
    int protocol;
    unsigned char *data;
    uint16_t length;
    struct dgram_batch *batch; /* non-NULL: this ring item is a burst's datagrams for
                                  the socket, delivered with one copy (GPU compaction) */
    struct offload *gnext;     /* (on the garbage list, see reclaim) */
};

/* The datagrams of one burst for one socket, in burst order, as the GPU's
 * compaction (rxg_process_mbufs_udp) hands them over: one allocation, one
 * memcpy of the socket's payload slice.  Each datagram reads as the offload
 * udp_process would have enqueued for it (udp.c:31-46): length = dgram_len,
 * the captured payload then zeros. */
struct dgram_meta {
    uint32_t sip, off; /* source address; payload offset in data */
    uint16_t sport, len, ncopy; /* source port; payload bytes (dgram_len - 8); captured ones */
};
struct dgram_batch {
    uint32_t n, next; /* datagrams; the next one to read */
    struct dgram_meta *meta;
    unsigned char *data;
};

/* ---- batch memory: each thread's cache of freed blocks, by size class ----
 * A burst allocates one or two batches per connection (its receive fragments,
 * its ACKs) or socket (its datagrams), and the protocol thread frees as many
 * (reclaim); glibc serves blocks of these sizes (0.2-1.5 KB) from its small
 * bins at 35-300 ns per call once its 7-entry per-size cache is exhausted
 * (a burst frees thousands at once), a free list here at a few ns.  Blocks up
 * to BP_CLASSES x BP_GRAN bytes, kept up to BP_KEEP per class and BP_BYTES in
 * all per thread; larger ones, and frees past the caps, go to malloc / free.
 * A thread's cache is released when it exits (bp_key) and by nstack_fini for
 * the calling thread. */
enum { BP_GRAN = 256, BP_CLASSES = 64, BP_KEEP = 16384 };
#define BP_BYTES (64ull << 20)
struct bp_hdr {
    uint32_t cls; /* 0: not cached (freed to malloc) */
    uint32_t pad;
    struct bp_hdr *next;
}; /* 16 B: the block keeps malloc's 16-B alignment */
static __thread struct bp_hdr *t_bp_head[BP_CLASSES];
static __thread uint32_t t_bp_n[BP_CLASSES];
static __thread uint64_t t_bp_bytes; /* bytes held by this thread's cache */
static pthread_key_t bp_key;
static pthread_once_t bp_once = PTHREAD_ONCE_INIT;
static void bp_drain(void) {
    for (int c = 0; c < BP_CLASSES; c++) {
        while (t_bp_head[c]) {
            struct bp_hdr *h = t_bp_head[c];
            t_bp_head[c] = h->next;
            free(h);
        }
        t_bp_n[c] = 0;
    }
    t_bp_bytes = 0;
}
static void bp_thread_exit(void *v) { (void)v, bp_drain(); }
static void bp_key_init(void) { (void)pthread_key_create(&bp_key, bp_thread_exit); }
static void *bp_alloc(size_t sz) {
    const size_t c = (sz + sizeof(struct bp_hdr) + BP_GRAN - 1) / BP_GRAN;
    struct bp_hdr *h;
    if (c < BP_CLASSES && t_bp_head[c]) {
        h = t_bp_head[c];
        t_bp_head[c] = h->next;
        t_bp_n[c]--;
        t_bp_bytes -= c * BP_GRAN;
        return h + 1;
    }
    h = malloc(c < BP_CLASSES ? c * BP_GRAN : sz + sizeof(*h));
    if (!h) return NULL;
    h->cls = c < BP_CLASSES ? (uint32_t)c : 0u;
    return h + 1;
}
static void bp_free(void *p) {
    if (!p) return;
    struct bp_hdr *h = (struct bp_hdr *)p - 1;
    const uint32_t c = h->cls;
    if (c && t_bp_n[c] < BP_KEEP && t_bp_bytes + c * BP_GRAN <= BP_BYTES) {
        if (!t_bp_n[c]) { /* (a thread's first cached block: its exit releases the cache) */
            pthread_once(&bp_once, bp_key_init);
            (void)pthread_setspecific(bp_key, (void *)1);
        }
        h->next = t_bp_head[c];
        t_bp_head[c] = h;
        t_bp_n[c]++;
        t_bp_bytes += c * BP_GRAN;
        return;
    }
    free(h);
}

/* Items the application threads are done with go back to the protocol
 * thread, which allocated them: freed there (reclaim, at its next burst
 * call), they stay in its malloc arena's fast paths instead of each free
 * taking the arena's lock against its next allocations (glibc frees a chunk
 * into the arena it came from), and the frames they hold (in-place receive)
 * are let go on the core that took them.  Lock-free: pushed one by one,
 * taken all at once. */
static __thread int t_proto; /* this thread makes the protocol loop's calls */
static _Atomic(struct offload *) g_off_garbage;

static void offload_free_now(struct offload *o) {
    if (!o) return;
    if (o->batch) { /* (one block: the item, the batch, its meta and data) */
        bp_free(o);
        return;
    }
    free(o->data);
    free(o);
}
static void offload_free(struct offload *o) {
    if (!o) return;
    if (t_proto) {
        offload_free_now(o);
        return;
    }
    struct offload *old = atomic_load_explicit(&g_off_garbage, memory_order_relaxed);
    do
        o->gnext = old;
    while (!atomic_compare_exchange_weak_explicit(&g_off_garbage, &old, o, memory_order_release,
                                                  memory_order_relaxed));
}

struct tcp_stream {
    int fd;
    uint32_t dip;
    uint8_t localmac[6];
    uint16_t dport;
    uint8_t protocol;
    uint16_t sport;
    uint32_t sip;
    uint32_t snd_nxt, rcv_nxt;
    int status;
    struct nring *sndbuf, *rcvbuf;
    uint32_t rq, sq;            /* fragments in rcvbuf / sndbuf (a batch item holds several) */
    /* what a reader touches, together: the lock, the receive ring, the state */
    pthread_mutex_t mutex;
    struct nring rcv_r;
    atomic_int ref;             /* the lists' reference + one per reader (cb_get / tcb_put) */
    int dead;                   /* unlinked (last ACK, nclose): readers return, the last
                                   put frees */
    uint32_t flow_id;           /* stable id in the GPU flow tables (verdict flow_id) */
    struct nring snd_r;
    struct tcp_stream *prev, *next;
    pthread_cond_t cond;
    pthread_cond_t accept_cond; /* naccept waits here, paired with g_lock */
};

struct frag_batch;
struct tcp_fragment {
    uint16_t sport, dport;
    uint32_t seqnum, acknum;
    uint8_t hdrlen_off, tcp_flags;
    uint16_t windows, cksum, tcp_urp;
    int optlen;
    uint32_t option[10];
    unsigned char *data;
    uint32_t length;
    struct frag_batch *batch; /* non-NULL: this ring item is a burst's fragments for the
                                 tcb, in one allocation (GPU segment sort) */
    rxg_mbuf *mb;             /* in-place delivery: data points into this mbuf's frame,
                                 held (refcnt) until the fragment's item is freed */
    struct tcp_fragment *gnext; /* (on the garbage list, see reclaim) */
};

/* The fragments one burst queues on one tcb (its receive fragments, or the
 * ACKs it sends), as the GPU's segment sort hands a connection's segments
 * over: one allocation holding the fragments and their payloads, one ring
 * item.  Each fragment reads as the one tcp_process would have queued on its
 * own (tcp.c:133-216); the tcb's rq / sq count fragments, not items, so the
 * rings keep their D_RING_SIZE-fragment capacity. */
struct frag_batch {
    struct tcp_fragment item; /* the ring item (item.batch = this batch) */
    uint32_t n, next;         /* fragments; the next one to read */
    struct tcp_fragment *frag;
    int32_t pl_ref;           /* >= 0: payloads point into the library's pinned buffer
                                 pl_ref, held (rxg_payload_hold) until the batch is freed */
};

/* ---- a tcb's fragment queues: logical fragments over ring items ---------- */
static rxg_ctx *g_ctx;
static atomic_llong g_pl_batches; /* batches holding a library payload buffer (stat 7) */
/* Backpressure for the two-thread arrangement: the batches queued per pooled
 * payload buffer, the buffer each delivery set's last burst used (the library
 * holds it until that set's next submit), and the drain_all calls running.
 * While an application thread drains, nstack_rx_burst waits (the stack's lock
 * released) for a pooled buffer to come free rather than have the library
 * hand out the set's own buffer, whose payloads would then be copied. */
static atomic_int g_pl_out[RXG_PAYLOAD_BUFS];
static int32_t g_set_ref[RXG_DELIVER_DEPTH];
static uint32_t g_next_set; /* the set the next submit takes (the library's round robin) */
static atomic_int g_drainers;
static pthread_mutex_t g_pl_mx = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_pl_cv = PTHREAD_COND_INITIALIZER;
static uint64_t g_pl_waits; /* submits that waited for a buffer (stat 11) */
static atomic_int g_pl_waiting; /* the protocol thread is in pl_wait_free */
/* drain_all's time, ns (stats 8-10): waiting for the id maps' lock (g_tab),
 * stepping aside for the protocol thread (0: no longer done), reading out
 * what it took from the blocks */
static atomic_llong g_drain_ns[3];
/* bursts delivered (nstack_rx_burst, nstack_deliver; stat 12): bumped with
 * release order after a burst's deliveries, so a polling application that
 * reads a new value (acquire) finds that burst's items in drain_all's look */
static atomic_ullong g_deliveries;
/* In-place TCP delivery (nstack_set_rx_inplace): a receive fragment whose
 * payload was captured whole points into its frame and holds the frame's mbuf
 * (refcnt@18, as rte_mbuf_refcnt_update) until the application has read it;
 * the put that drops the count to 0 hands the mbuf to g_mb_release (the
 * mempool's free, rte_pktmbuf_free). */
static int g_inplace;
/* Receive coalescing (nstack_set_rx_gro): the window in bytes, 0 = off; a
 * connection's in-sequence PSH|ACK trains arrive as runs (rxg_tcp_run) and
 * each run of more than one segment makes one receive fragment and one ACK.
 * g_gro_absorbed (stat 15): segments that went into a preceding segment's
 * fragment. */
static uint32_t g_gro;
static uint64_t g_gro_absorbed;
/* Sequence ordering (nstack_set_rx_order): a burst's segments reach each
 * connection in seq order (RXG_DLV_TCP_ORDER on the device paths,
 * rxg_tcp_order_host in nstack_deliver).  g_order_moved (stat 16): records
 * that changed position. */
static int g_order;
static uint64_t g_order_moved;
/* Stream assembly (nstack_set_rx_assemble): a connection's segments of a burst
 * are ordered, then assembled into contiguous byte ranges with duplicates
 * dropped, overlaps trimmed and a stop at every hole (RXG_DLV_TCP_ASSEMBLE on
 * the device paths; rxg_tcp_order_host, then rxg_tcp_assemble_host in
 * nstack_deliver), and every stream is aligned with rcv_nxt before anything is
 * queued (the host rule: rxgpu.h, "TCP stream assembly").  g_asm_dup (stat
 * 19): payload bytes discarded as already received; g_asm_hole (stat 20):
 * streams ignored behind a hole. */
static int g_assemble;
static uint64_t g_asm_dup, g_asm_hole;
/* a burst's streams as deliver_tcp_sorted takes them (NULL: assembly off);
 * the records then carry ncopy = take */
struct asm_view {
    const rxg_tcp_stream *st;
    uint32_t n;
};
/* The entropy flood detector (nstack_set_rx_ddos): every received frame goes
 * through it in arrival order (RXG_DLV_DDOS on the device paths, rxg_ddos_host
 * with g_ddos_state in nstack_deliver).  Detection only: nothing else reads
 * what it finds.  g_ddos_acc: what nstack_ddos_status reports (alarm_frames
 * is stat 17, rises stat 18). */
static int g_ddos;
static double g_ddos_thresh = RXG_DDOS_DEFAULT_THRESH;
static rxg_ddos_state g_ddos_state;
static nstack_ddos g_ddos_acc;
/* one burst's summary into the running status (g_lock held); a burst the
 * detector did not see has a zeroed summary */
static void ddos_account(const rxg_ddos_summary *s) {
    if (!s->frames_seen) return;
    g_ddos_acc.frames_seen = s->frames_seen;
    g_ddos_acc.alarm = s->flag;
    g_ddos_acc.rises += s->rises;
    g_ddos_acc.falls += s->falls;
    g_ddos_acc.alarm_frames += s->alarm_frames;
    g_ddos_acc.undef_frames += s->undef_frames;
    g_ddos_acc.last_stat = s->last_stat;
}
/* the frames of a host-verdict burst through rxg_ddos_host (g_lock held):
 * packed at 16-B aligned offsets first, since mbuf data lies anywhere (out of
 * memory: the burst goes unseen) */
static void ddos_host_burst(rxg_mbuf *const *m, uint32_t n) {
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < n; i++) bytes += ((uint64_t)m[i]->data_len + 15u) & ~15ull;
    uint8_t *pk = malloc(bytes ? bytes : 16);
    uint32_t *off = malloc((size_t)n * sizeof(*off));
    uint16_t *len = malloc((size_t)n * sizeof(*len));
    if (pk && off && len && (bytes >> 4) <= 0xFFFFFFFFull) {
        uint64_t pos = 0;
        for (uint32_t i = 0; i < n; i++) {
            off[i] = (uint32_t)(pos >> 4);
            len[i] = m[i]->data_len;
            memcpy(pk + pos, (const uint8_t *)m[i]->buf_addr + m[i]->data_off, len[i]);
            pos += ((uint64_t)len[i] + 15u) & ~15ull;
        }
        rxg_ddos_summary sum;
        if (rxg_ddos_host(pk, off, len, n, 4, g_ddos_thresh, &g_ddos_state, NULL, NULL, NULL, &sum) ==
            RXG_OK)
            ddos_account(&sum);
    }
    free(pk), free(off), free(len);
}
/* SYN cookies (nstack_set_syncookies; the rule: rxgpu.h, "SYN cookies"): a
 * listener keeps no state for a SYN.  Each burst is judged once (K7 with
 * RXG_DLV_SYNCOOKIE on the device paths, rxg_syncookie_host in nstack_deliver):
 * a SYN's descriptor waits in s_ck_tx for the next nstack_tx_burst, a
 * handshake ACK whose cookie verifies creates its tcb ESTABLISHED when it
 * reaches the LISTEN handler, any other ACK is counted.  A frame whose burst
 * result cannot be used (verdicts of an older snapshot, a lookup made again on
 * the live list that found another block, the option switched on between a
 * submit and its delivery) is judged alone, by the same host call.  g_ck_mode:
 * 0 off, 1 on, 2 on while the flood detector's alarm is up (as it stood before
 * the burst).  All of it under g_lock. */
#define CK_JUDGE 0xFFu         /* no burst status for this frame */
#define CK_TX_MAX (1u << 16)   /* SYN-ACKs waiting for a TX burst; a SYN past it goes unanswered */
static int g_ck_mode;
static rxg_ck_params g_ck_p;
static uint32_t g_ck_pin = 0xFFFFFFFFu; /* nstack_syncookie_tick (all ones: the clock) */
static uint64_t g_ck_syn, g_ck_acc, g_ck_rej; /* nstack_syncookie_stats */
static uint32_t *s_ck_mask;    /* one bit per tcb id: the listeners */
static uint32_t s_ck_mask_cap, g_ck_space;
static rxg_txd *s_ck_tx;       /* the waiting SYN-ACKs: [g_ck_tx_head, g_ck_tx_n) */
static uint32_t s_ck_tx_cap, g_ck_tx_head, g_ck_tx_n;
static int g_ck_on;            /* the burst being delivered is judged */
static const uint8_t *g_ck_st; /* its per-frame statuses; NULL: frame by frame */
static uint8_t g_ck_cur;       /* the status of the frame in tcp_dispatch */
static uint8_t *s_ck_hst;      /* the host path's statuses, descriptors and frame heads */
static rxg_txd *s_ck_htx;
static uint8_t *s_ck_hpk;
static uint32_t *s_ck_hoff;
static uint16_t *s_ck_hlen;
static uint32_t s_ck_hcap;

static int ck_active(void) {
    return g_ck_mode == 1 || (g_ck_mode == 2 && g_ddos && g_ddos_acc.alarm);
}
static uint32_t ck_now(void) {
    if (g_ck_pin != 0xFFFFFFFFu) return g_ck_pin;
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint32_t)((uint64_t)ts.tv_sec / 64u);
}
/* k descriptors behind the waiting ones (what does not fit is dropped) */
static void ck_tx_push(const rxg_txd *d, uint32_t k) {
    if (g_ck_tx_head == g_ck_tx_n) g_ck_tx_head = g_ck_tx_n = 0;
    const uint32_t have = g_ck_tx_n - g_ck_tx_head;
    if (k > CK_TX_MAX - have) k = CK_TX_MAX - have;
    if (!k) return;
    if (g_ck_tx_n + k > s_ck_tx_cap) {
        if (g_ck_tx_head) {
            memmove(s_ck_tx, s_ck_tx + g_ck_tx_head, (size_t)have * sizeof(*d));
            g_ck_tx_head = 0, g_ck_tx_n = have;
        }
        if (have + k > s_ck_tx_cap) {
            uint32_t cap = s_ck_tx_cap ? s_ck_tx_cap : 256;
            while (cap < have + k) cap *= 2;
            rxg_txd *t = realloc(s_ck_tx, (size_t)cap * sizeof(*t));
            if (!t) return;
            s_ck_tx = t, s_ck_tx_cap = cap;
        }
    }
    memcpy(s_ck_tx + g_ck_tx_n, d, (size_t)k * sizeof(*d));
    g_ck_tx_n += k;
}
/* a judged burst's descriptors and totals taken over */
static void ck_take(const rxg_txd *txd, const uint32_t tot[4]) {
    ck_tx_push(txd, tot[0]);
    g_ck_syn += tot[0];
    g_ck_rej += tot[2];
}
/* one frame judged alone, as a candidate: its status, a SYN's descriptor in *d */
static uint8_t ck_judge_frame(const uint8_t *f, uint32_t cap, rxg_txd *d) {
    uint8_t head[64] __attribute__((aligned(16)));
    memset(head, 0, sizeof(head));
    memcpy(head, f, cap < 64u ? cap : 64u);
    const uint32_t off = 0, mask = 1u;
    const uint16_t len = (uint16_t)(cap < 65535u ? cap : 65535u);
    rxg_verdict v;
    memset(&v, 0, sizeof(v));
    v.cls = RXG_CLS_TCP, v.rc = RXG_RC_OK;
    uint8_t st = 0;
    uint32_t tot[4];
    if (rxg_syncookie_host(head, &off, &len, 1, 4, &v, &mask, 1, &g_ck_p, &st, d, tot) != RXG_OK)
        return 0;
    return st;
}
/* a host-verdict burst through rxg_syncookie_host: the frames' first 64
 * bytes packed at 64-B slots (the rule reads no byte past 47).  Sets g_ck_st;
 * out of memory: the frames are judged one by one */
static void ck_host_burst(rxg_mbuf *const *m, uint32_t n, const rxg_verdict *v) {
    if (n > s_ck_hcap) {
        free(s_ck_hst), free(s_ck_htx), free(s_ck_hpk), free(s_ck_hoff), free(s_ck_hlen);
        s_ck_hst = malloc(n), s_ck_htx = malloc((size_t)n * sizeof(rxg_txd));
        s_ck_hpk = aligned_alloc(64, (size_t)n * 64u);
        s_ck_hoff = malloc((size_t)n * sizeof(uint32_t)), s_ck_hlen = malloc((size_t)n * sizeof(uint16_t));
        s_ck_hcap = s_ck_hst && s_ck_htx && s_ck_hpk && s_ck_hoff && s_ck_hlen ? n : 0;
        if (!s_ck_hcap) {
            free(s_ck_hst), free(s_ck_htx), free(s_ck_hpk), free(s_ck_hoff), free(s_ck_hlen);
            s_ck_hst = NULL, s_ck_htx = NULL, s_ck_hpk = NULL, s_ck_hoff = NULL, s_ck_hlen = NULL;
            return;
        }
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = m[i]->data_len < 64u ? m[i]->data_len : 64u;
        memcpy(s_ck_hpk + (size_t)i * 64u, (const uint8_t *)m[i]->buf_addr + m[i]->data_off, c);
        s_ck_hoff[i] = i * 4u; /* 16-B units */
        s_ck_hlen[i] = m[i]->data_len;
    }
    uint32_t tot[4];
    if (rxg_syncookie_host(s_ck_hpk, s_ck_hoff, s_ck_hlen, n, 4, v, s_ck_mask, g_ck_space, &g_ck_p,
                           s_ck_hst, s_ck_htx, tot) != RXG_OK)
        return;
    ck_take(s_ck_htx, tot);
    g_ck_st = s_ck_hst;
}
/* The L2 responder (nstack_set_l2_respond; the rule: rxgpu.h, "L2 responder"):
 * ARP requests for the local address and echo requests to it are answered.
 * Each burst is judged once (K8 with RXG_DLV_L2 on the device paths,
 * rxg_l2_host in nstack_deliver); a frame whose burst result cannot be used
 * (verdicts of an older snapshot, the option switched on between a submit and
 * its delivery) is judged alone, by the same host call.  The answers are
 * complete frames: copies wait in a bounded queue for the front of the next
 * nstack_tx_burst.  All of it under g_lock. */
#define L2_Q_FRAMES 1024u            /* answers waiting for a TX burst ... */
#define L2_Q_BYTES (2u << 20)        /* ... and their 64-B slots; past either an answer is dropped */
#define L2_BURST_BYTES (256u << 10)  /* the device paths' answer room per burst (rxg_l2_set) */
static int g_l2;
static uint64_t g_l2_arp, g_l2_echo, g_l2_drop, g_l2_bad; /* stat 21-24 */
static struct l2_ans {
    uint8_t *b;
    uint32_t len;
} s_l2q[L2_Q_FRAMES];                /* a ring: [g_l2q_head, g_l2q_head + g_l2q_n) */
static uint32_t g_l2q_head, g_l2q_n;
static uint64_t g_l2q_bytes;
static uint8_t *s_l2_one;            /* the answer of a frame judged alone */
static uint32_t g_local_ip;          /* nstack_set_local */
static uint8_t g_local_mac[6];

static void l2_params_now(rxg_l2_params *p) {
    memset(p, 0, sizeof(*p));
    p->nlocal = g_local_ip ? 1u : 0u;
    p->local[0].ip = g_local_ip;
    memcpy(p->local[0].mac, g_local_mac, 6);
}
/* the local address and the per-burst room to the context (g_lock held) */
static int l2_sync(void) {
    if (!g_l2 || !g_ctx) return RXG_OK;
    rxg_l2_params p;
    l2_params_now(&p);
    return rxg_l2_set(g_ctx, &p, L2_BURST_BYTES);
}
static void l2_push(const uint8_t *f, uint32_t len, uint8_t st) {
    const uint64_t slot = ((uint64_t)len + 63u) & ~63ull;
    uint8_t *b = g_l2q_n < L2_Q_FRAMES && g_l2q_bytes + slot <= L2_Q_BYTES ? malloc(len) : NULL;
    if (!b) {
        g_l2_drop++;
        return;
    }
    memcpy(b, f, len);
    struct l2_ans *a = &s_l2q[(g_l2q_head + g_l2q_n) % L2_Q_FRAMES];
    a->b = b, a->len = len;
    g_l2q_n++, g_l2q_bytes += slot;
    st == RXG_L2_ARP_REQ ? g_l2_arp++ : g_l2_echo++;
}
static void l2_q_clear(void) {
    for (; g_l2q_n; g_l2q_n--, g_l2q_head = (g_l2q_head + 1) % L2_Q_FRAMES) free(s_l2q[g_l2q_head].b);
    g_l2q_head = 0, g_l2q_bytes = 0;
}
/* a judged burst's answers and totals taken over; an answered frame whose
 * answer the burst had no room for counts as dropped */
static void l2_take(const uint8_t *status, const uint8_t *frames, const uint32_t *roff,
                    const uint16_t *rlen, const uint32_t *rsrc, uint32_t nans, const uint32_t tot[6]) {
    for (uint32_t k = 0; k < nans; k++) l2_push(frames + ((uint64_t)roff[k] << 6), rlen[k], status[rsrc[k]]);
    g_l2_drop += (uint64_t)tot[0] + tot[2] - nans;
    g_l2_bad += tot[3];
}
/* the frames of a burst judged one by one, each alone, by rxg_l2_host (the
 * host-verdict path, and a device burst whose result cannot be used) */
static void l2_host_frames(rxg_mbuf *const *m, uint32_t n, const rxg_verdict *v) {
    if (!s_l2_one && !(s_l2_one = malloc(65536u + 64u))) return;
    rxg_l2_params p;
    l2_params_now(&p);
    for (uint32_t i = 0; i < n; i++) {
        if (v[i].cls != RXG_CLS_ARP && v[i].cls != RXG_CLS_IPV4_OTHER) continue;
        const uint32_t off = 0;
        const uint16_t len = m[i]->data_len;
        uint8_t st = 0;
        uint32_t roff, rsrc = 0, tot[6];
        uint16_t rlen;
        if (rxg_l2_host((const uint8_t *)m[i]->buf_addr + m[i]->data_off, &off, &len, 1, 4, &v[i], &p,
                        &st, s_l2_one, 65536u + 64u, &roff, &rlen, &rsrc, tot) != RXG_OK)
            continue;
        l2_take(&st, s_l2_one, &roff, &rlen, &rsrc, tot[4], tot);
    }
}
/* the delivery flags the options ask for (g_lock held) */
static uint32_t dlv_flags(void) {
    return (g_inplace ? RXG_DLV_TCP_IN_PLACE : g_gro ? RXG_DLV_TCP_GRO : 0u) |
           (g_order ? RXG_DLV_TCP_ORDER : 0u) | (g_ddos ? RXG_DLV_DDOS : 0u) |
           (g_assemble ? RXG_DLV_TCP_ASSEMBLE : 0u) | (g_ck_mode ? RXG_DLV_SYNCOOKIE : 0u) |
           (g_l2 ? RXG_DLV_L2 : 0u);
}
static void (*g_mb_release)(rxg_mbuf *m, void *arg);
static void *g_mb_arg;
static inline void mb_get(rxg_mbuf *m) { __atomic_fetch_add(&m->refcnt, 1, __ATOMIC_RELAXED); }
static inline void mb_put(rxg_mbuf *m) {
    if (__atomic_fetch_sub(&m->refcnt, 1, __ATOMIC_ACQ_REL) == 1 && g_mb_release)
        g_mb_release(m, g_mb_arg);
}
static _Atomic(struct tcp_fragment *) g_frag_garbage;
static void frag_item_free_now(struct tcp_fragment *f) {
    if (f->batch) {
        for (uint32_t j = 0; j < f->batch->n; j++)
            if (f->batch->frag[j].mb) mb_put(f->batch->frag[j].mb);
        if (f->batch->pl_ref >= 0) {
            rxg_payload_release(g_ctx, f->batch->pl_ref);
            atomic_fetch_sub_explicit(&g_pl_batches, 1, memory_order_relaxed);
            if (atomic_fetch_sub_explicit(&g_pl_out[f->batch->pl_ref], 1, memory_order_acq_rel) == 1 &&
                atomic_load_explicit(&g_drainers, memory_order_relaxed)) {
                pthread_mutex_lock(&g_pl_mx); /* the last batch on that buffer */
                pthread_cond_broadcast(&g_pl_cv);
                pthread_mutex_unlock(&g_pl_mx);
            }
        }
        bp_free(f->batch); /* (fragments and payloads live in the batch's block) */
    } else {
        if (f->mb)
            mb_put(f->mb);
        else
            free(f->data);
        free(f);
    }
}
static void frag_item_free(struct tcp_fragment *f) {
    if (t_proto) {
        frag_item_free_now(f);
        return;
    }
    const int pooled = f->batch && f->batch->pl_ref >= 0;
    struct tcp_fragment *old = atomic_load_explicit(&g_frag_garbage, memory_order_relaxed);
    do
        f->gnext = old;
    while (!atomic_compare_exchange_weak_explicit(&g_frag_garbage, &old, f, memory_order_seq_cst,
                                                  memory_order_relaxed));
    /* a batch holding a pooled buffer: wake a protocol thread waiting for one
     * in pl_wait_free, which reclaims it at once (it waited for
     * its next 1-ms timed wakeup).  The push and this load are seq_cst, as
     * are the waiter's flag store and its look at the list: either this sees
     * the flag or the waiter sees the push */
    if (pooled && atomic_load_explicit(&g_pl_waiting, memory_order_seq_cst)) {
        pthread_mutex_lock(&g_pl_mx);
        pthread_cond_broadcast(&g_pl_cv);
        pthread_mutex_unlock(&g_pl_mx);
    }
}
/* the protocol thread frees what the application threads let go of */
static void reclaim(void) {
    t_proto = 1;
    struct tcp_fragment *f = atomic_exchange_explicit(&g_frag_garbage, NULL, memory_order_acquire);
    while (f) {
        struct tcp_fragment *nx = f->gnext;
        frag_item_free_now(f);
        f = nx;
    }
    struct offload *o = atomic_exchange_explicit(&g_off_garbage, NULL, memory_order_acquire);
    while (o) {
        struct offload *nx = o->gnext;
        offload_free_now(o);
        o = nx;
    }
}
/* The queue counters (a tcb's rq / sq, a UDP socket's queued) are written
 * under the block's mutex and read without it by drain_all's look for work
 * (drain_impl): relaxed atomic stores and that relaxed load, so the look is
 * no data race (holders of the mutex read them plainly). */
static inline uint32_t cnt_peek(const uint32_t *c) { return __atomic_load_n(c, __ATOMIC_RELAXED); }
static inline void cnt_set(uint32_t *c, uint32_t v) { __atomic_store_n(c, v, __ATOMIC_RELAXED); }

/* a standalone fragment at the tail (ring full: -ENOBUFS, the caller keeps it) */
static int tq_push(struct nring *r, uint32_t *cnt, struct tcp_fragment *f) {
    if (*cnt >= D_RING_SIZE || ring_enqueue(r, f)) return -ENOBUFS;
    cnt_set(cnt, *cnt + 1);
    return 0;
}
/* the logical head, or NULL */
static struct tcp_fragment *tq_front(struct nring *r) {
    struct tcp_fragment *f;
    if (ring_peek(r, (void **)&f)) return NULL;
    return f->batch ? &f->batch->frag[f->batch->next] : f;
}
/* fragment k (0 = head), or NULL */
static struct tcp_fragment *tq_at(struct nring *r, uint32_t k) {
    void *p;
    for (uint32_t i = 0; ring_peek_at(r, i, &p) == 0; i++) {
        struct tcp_fragment *f = p;
        const uint32_t left = f->batch ? f->batch->n - f->batch->next : 1u;
        if (k < left) return f->batch ? &f->batch->frag[f->batch->next + k] : f;
        k -= left;
    }
    return NULL;
}
/* drop the head fragment and its data */
static void tq_pop(struct nring *r, uint32_t *cnt) {
    struct tcp_fragment *f;
    if (ring_peek(r, (void **)&f)) return;
    cnt_set(cnt, *cnt - 1);
    if (f->batch && ++f->batch->next < f->batch->n) return;
    ring_dequeue(r, (void **)&f);
    frag_item_free(f);
}
/* the head fragment taken out as a standalone one the caller owns (a batch
 * member is copied out), or NULL */
static struct tcp_fragment *tq_detach(struct nring *r, uint32_t *cnt) {
    struct tcp_fragment *f;
    if (ring_peek(r, (void **)&f)) return NULL;
    if (!f->batch) {
        ring_dequeue(r, (void **)&f);
        cnt_set(cnt, *cnt - 1);
        return f;
    }
    const struct tcp_fragment *m = &f->batch->frag[f->batch->next];
    struct tcp_fragment *c = calloc(1, sizeof(*c));
    if (!c) return NULL;
    *c = *m;
    c->batch = NULL;
    c->data = NULL;
    c->mb = NULL; /* (a copy: the batch keeps its hold on the frame until it is freed) */
    if (m->data) {
        c->data = malloc((size_t)m->length + 1);
        if (!c->data) {
            free(c);
            return NULL;
        }
        memcpy(c->data, m->data, m->length);
        c->data[m->length] = 0;
    }
    tq_pop(r, cnt);
    return c;
}
static void tq_clear(struct nring *r, uint32_t *cnt) {
    void *p;
    while (ring_dequeue(r, &p) == 0) frag_item_free(p);
    cnt_set(cnt, 0);
}

#define LL_ADD(item, list)                                                                         \
    do {                                                                                           \
        (item)->prev = NULL;                                                                       \
        (item)->next = (list);                                                                     \
        if ((list) != NULL) (list)->prev = (item);                                                 \
        (list) = (item);                                                                           \
    } while (0)

#define LL_REMOVE(item, list)                                                                      \
    do {                                                                                           \
        if ((item)->prev != NULL) (item)->prev->next = (item)->next;                               \
        if ((item)->next != NULL) (item)->next->prev = (item)->prev;                               \
        if ((list) == (item)) (list) = (item)->next;                                               \
        (item)->prev = (item)->next = NULL;                                                        \
    } while (0)

_Static_assert(sizeof(struct offload) % 8 == 0, "a datagram batch follows its item in one block");
_Static_assert(offsetof(struct localhost, protocol) == offsetof(struct tcp_stream, protocol),
               "get_hostinfo_fromfd reads either block's protocol byte at one offset");

/* ---- control-block lifetime ----------------------------------------------
 * A block carries a reference count: one for being linked (lists, id and fd
 * maps, flow tables) and one per application call that uses it after the
 * stack's lock is released (naccept takes its reference under g_lock;
 * nrecv / nrecvfrom / nsendto / drain_all under g_tab, the id maps' lock:
 * either way where the block is still linked).
 * Freeing a block (nclose, the last ACK of LAST_ACK) unlinks it under the
 * lock, marks it dead and wakes its waiters, then drops the linked reference;
 * whoever drops the last one frees the memory.  So a reader blocked in nrecv
 * on a connection another thread closes wakes up and returns instead of
 * waiting on freed memory (the reference has that race: tcp.c:312-331
 * frees the tcb under a concurrent nrecv, common.c:476-481). */
static void udp_destroy(struct localhost *h) {
    void *p;
    while (ring_dequeue(h->rcvbuf, &p) == 0) offload_free(p);
    while (ring_dequeue(h->sndbuf, &p) == 0) {
        free(((struct offload *)p)->data);
        free(p);
    }
    ring_free(h->rcvbuf);
    ring_free(h->sndbuf);
    pthread_cond_destroy(&h->cond);
    pthread_mutex_destroy(&h->mutex);
    free(h);
}
static void tcb_destroy(struct tcp_stream *s) {
    tq_clear(s->rcvbuf, &s->rq);
    tq_clear(s->sndbuf, &s->sq);
    ring_free(s->rcvbuf);
    ring_free(s->sndbuf);
    pthread_cond_destroy(&s->cond);
    pthread_cond_destroy(&s->accept_cond);
    pthread_mutex_destroy(&s->mutex);
    free(s);
}
static inline void cb_ref_init(atomic_int *ref) { atomic_init(ref, 1); }
static inline void cb_get(atomic_int *ref) { atomic_fetch_add_explicit(ref, 1, memory_order_relaxed); }
static void udp_put(struct localhost *h) {
    if (atomic_fetch_sub_explicit(&h->ref, 1, memory_order_acq_rel) == 1) udp_destroy(h);
}
static void tcb_put(struct tcp_stream *s) {
    if (atomic_fetch_sub_explicit(&s->ref, 1, memory_order_acq_rel) == 1) tcb_destroy(s);
}
/* a block of either kind (the protocol byte sits at the same offset in both,
 * as get_hostinfo_fromfd assumes, common.c:111-143) */
static void cb_put(void *cb) {
    if (((struct localhost *)cb)->protocol == IPPROTO_UDP)
        udp_put(cb);
    else
        tcb_put(cb);
}
/* the block is unlinked (g_lock held): readers wake and return; the linked
 * reference goes */
static void udp_kill(struct localhost *h) {
    pthread_mutex_lock(&h->mutex);
    h->dead = 1;
    pthread_cond_broadcast(&h->cond);
    pthread_mutex_unlock(&h->mutex);
    udp_put(h);
}
static void tcb_kill(struct tcp_stream *s) {
    pthread_mutex_lock(&s->mutex);
    s->dead = 1;
    pthread_cond_broadcast(&s->cond);
    pthread_mutex_unlock(&s->mutex);
    pthread_cond_broadcast(&s->accept_cond); /* (naccept waits with g_lock, held here) */
    tcb_put(s);
}

/* ---- process-wide state (netfamily.c:16-18) ----------------------------- */
static struct localhost *g_pstHost;
static struct tcp_stream *g_tcb_set;
static unsigned char g_ucFdTable[D_MAX_FD_COUNT / 8 + 1];
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER; /* guards lists + snapshot */
/* The id and descriptor maps (s_udp_cb / s_tcb_cb, g_fd_cb) are written only
 * with g_lock held AND under g_tab, so an application call can look a block
 * up and take its reference under g_tab alone — a lock held for a few stores
 * — instead of waiting behind the protocol thread's whole delivery, which
 * holds g_lock (lock order: g_lock, then g_tab). */
static pthread_mutex_t g_tab = PTHREAD_MUTEX_INITIALIZER;
static int g_dirty = 1;       /* the creation-order export (nstack_flows) is stale */
static uint64_t g_snap_gen; /* bumped whenever a lookup result may change */
static int g_burst_stale;   /* the burst's verdicts were made for an older snapshot */
static uint64_t g_stat[5];
static unsigned int g_isn_seed; /* tcp_stream_create seeds rand_r with time(NULL) (tcp.c:30-31) */

/* ARP table and local identity (common.c:145-204; gLocalIp / g_stCpuMac,
 * netfamily.c:11,13,415) */
struct arp_entry {
    uint32_t ip;
    uint8_t mac[6];
    struct arp_entry *prev, *next;
};
static struct arp_entry *g_arp; /* head-inserted (LL_ADD, common.c:195) */
static const uint8_t k_default_arp_mac[6] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF}; /* netfamily.c:20 */
static int g_burst_mutated;     /* the tcb list changed during this burst's delivery */
static int g_rx_in_flight;      /* nstack_rx_burst waits for the GPU (g_lock released) */
static uint32_t g_pend_n;      /* bursts nstack_rx_submit queued, not yet completed */
struct rx_pend {
    rxg_mbuf *const *m;
    uint32_t n;
    int *rc_out;
    rxg_verdict *v_out;
    rxg_verdict *v; /* the verdicts (the library's copy out lands here) */
    uint32_t v_cap;
    uint8_t *handled;
    uint32_t h_cap;
    rxg_delivery d;
    uint64_t gen0;   /* g_snap_gen at the submit */
    double lib_ms;   /* the library's time for this burst (submit, wait) */
    int waited, wrc; /* rxg_deliver_wait done, its result */
    float gms[8];    /* its phase times */
};
static struct rx_pend g_pend[RXG_DELIVER_DEPTH];
static uint32_t g_pend_head; /* the oldest pending burst */
static void pend_wait(struct rx_pend *p);
/* The protocol thread's (rx / tx bursts) hold of the stack's lock.  No
 * application loop takes g_lock any more (drain_all and the receive calls
 * look blocks up under g_tab), so nothing has to step aside for it. */
static void proto_lock(void) { pthread_mutex_lock(&g_lock); }
/* bursts of at least 2 * g_half_min frames run as two halves in flight
 * (nstack_set_halves; 0 = never) */
static uint32_t g_half_min;
static uint64_t g_stale_parts; /* burst halves delivered against changed lists */
static uint64_t g_copied_bytes; /* TCP payload bytes copied on the host (stat 6) */
static int g_udp_done;          /* this burst's UDP datagrams went out as batches */

/* the control block of each stable flow id (NULL: free id).  Blocks are
 * registered with the GPU flow tables as they are created, changed and freed
 * (rxg_flows_add / update / remove: the incremental path, committed with the
 * next burst), never by rebuilding the tables. */
static struct localhost **s_udp_cb;
static uint32_t s_udp_cap;
static struct tcp_stream **s_tcb_cb;
static uint32_t s_tcb_cap;
/* export (nstack_flows / nstack_flow_ids): the lists in creation order */
static rxg_udp_sock *s_udp;
static uint32_t *s_udp_id;
static uint32_t s_nu, s_udp_xcap;
static rxg_tcb *s_tcb;
static uint32_t *s_tcb_id;
static uint32_t s_nt, s_tcb_xcap;
static rxg_verdict *s_v;
static uint32_t s_v_cap;
static uint8_t *s_handled; /* per frame of the burst: delivered by the segment sort path */
static uint32_t s_handled_cap;

static int get_fd_frombitmap(void) { /* common.c:72-85 */
    for (int fd = D_DEFAULT_FD_NUM; fd < D_MAX_FD_COUNT; fd++)
        if ((g_ucFdTable[fd / 8] & (0x1 << (fd % 8))) == 0) {
            g_ucFdTable[fd / 8] |= (0x1 << (fd % 8));
            return fd;
        }
    return -1;
}

static int set_fd_frombitmap(int fd) { /* common.c:87-95 */
    if (fd < 0 || fd >= D_MAX_FD_COUNT) return -1;
    g_ucFdTable[fd / 8] &= ~(0x1 << (fd % 8));
    return 0;
}

/* common.c:111-143 (loop advances correctly here): the first block with the
 * fd, UDP list first, each newest first.  The walk's answer per fd is kept
 * in g_fd_cb and refreshed whenever a block with that fd is created, given
 * the fd (naccept), or freed, so the socket calls look their descriptor up
 * in O(1) instead of walking up to 1024 blocks per nrecvfrom. */
static void *g_fd_cb[D_MAX_FD_COUNT];
static uint32_t g_fd_nblk[D_MAX_FD_COUNT]; /* live blocks carrying each fd */

static void fd_refresh(int fd) {
    if (fd < 0 || fd >= D_MAX_FD_COUNT) return;
    void *cb = NULL;
    for (struct localhost *h = g_pstHost; h && !cb; h = h->next)
        if (h->fd == fd) cb = h;
    for (struct tcp_stream *s = g_tcb_set; s && !cb; s = s->next)
        if (s->fd == fd) cb = s;
    pthread_mutex_lock(&g_tab);
    g_fd_cb[fd] = cb;
    pthread_mutex_unlock(&g_tab);
}

/* a block just took fd (nsocket, naccept): it is the newest of its list, so
 * it is the answer unless it is a tcb and a UDP block holds the fd (the walk
 * looks at the UDP list first).  The protocol byte sits at the same offset in
 * both blocks (as the reference's get_hostinfo_fromfd assumes). */
static void fd_add(int fd, void *cb) {
    if (fd < 0 || fd >= D_MAX_FD_COUNT) return;
    g_fd_nblk[fd]++;
    const void *cur = g_fd_cb[fd];
    if (!cur || ((const struct localhost *)cb)->protocol == IPPROTO_UDP ||
        ((const struct localhost *)cur)->protocol != IPPROTO_UDP) {
        pthread_mutex_lock(&g_tab);
        g_fd_cb[fd] = cb;
        pthread_mutex_unlock(&g_tab);
    }
}
/* block cb (already unlinked) carried fd and is freed: O(1) unless it was the
 * answer and another block still carries the fd (then the walk) */
static void fd_del(int fd, const void *cb) {
    if (fd < 0 || fd >= D_MAX_FD_COUNT) return;
    if (g_fd_nblk[fd]) g_fd_nblk[fd]--;
    if (g_fd_cb[fd] != cb) return;
    if (!g_fd_nblk[fd]) {
        pthread_mutex_lock(&g_tab);
        g_fd_cb[fd] = NULL;
        pthread_mutex_unlock(&g_tab);
    } else {
        fd_refresh(fd);
    }
}

/* an application call's lookup: the block with this descriptor, referenced
 * (cb_get), or NULL; under g_tab only (see g_tab) */
static void *fd_get_ref(int fd) {
    if (fd < 0 || fd >= D_MAX_FD_COUNT) return NULL;
    pthread_mutex_lock(&g_tab);
    void *cb = g_fd_cb[fd];
    if (cb)
        cb_get(((struct localhost *)cb)->protocol == IPPROTO_UDP ? &((struct localhost *)cb)->ref
                                                                  : &((struct tcp_stream *)cb)->ref);
    pthread_mutex_unlock(&g_tab);
    return cb;
}

static void *get_hostinfo_fromfd(int fd) {
    return fd >= 0 && fd < D_MAX_FD_COUNT ? g_fd_cb[fd] : NULL;
}

/* common.c:58-70 */
static struct tcp_stream *get_accept_tcb(uint16_t dport) {
    for (struct tcp_stream *apt = g_tcb_set; apt; apt = apt->next)
        if (dport == apt->dport && apt->fd == -1) return apt;
    return NULL;
}

static int grow(void **p, uint32_t *cap, uint32_t need, size_t elem) {
    if (*cap >= need && *p) return 0;
    uint32_t c = *cap ? *cap : 64;
    while (c < need) c *= 2;
    void *q = realloc(*p, (size_t)c * elem);
    if (!q) return -1;
    *p = q;
    *cap = c;
    return 0;
}

/* the creation-order export of the lists (g_lock held) */
static int snapshot(void) {
    uint32_t nu = 0, nt = 0;
    struct localhost *h, *hlast = NULL;
    struct tcp_stream *s, *slast = NULL;
    for (h = g_pstHost; h; h = h->next) nu++, hlast = h;
    for (s = g_tcb_set; s; s = s->next) nt++, slast = s;
    uint32_t cu = s_udp_xcap, ct = s_tcb_xcap;
    if (grow((void **)&s_udp, &s_udp_xcap, nu, sizeof(rxg_udp_sock))) return RXG_ENOMEM;
    if (grow((void **)&s_udp_id, &cu, nu, sizeof(uint32_t))) return RXG_ENOMEM;
    if (grow((void **)&s_tcb, &s_tcb_xcap, nt, sizeof(rxg_tcb))) return RXG_ENOMEM;
    if (grow((void **)&s_tcb_id, &ct, nt, sizeof(uint32_t))) return RXG_ENOMEM;
    uint32_t i = 0;
    for (h = hlast; h; h = h->prev, i++) { /* tail = oldest */
        s_udp[i].localip = h->localip;
        s_udp[i].localport = h->localport;
        s_udp[i].protocol = h->protocol;
        s_udp[i]._pad = 0;
        s_udp_id[i] = h->flow_id;
    }
    i = 0;
    for (s = slast; s; s = s->prev, i++) {
        s_tcb[i].sip = s->sip;
        s_tcb[i].dip = s->dip;
        s_tcb[i].sport = s->sport;
        s_tcb[i].dport = s->dport;
        s_tcb[i].status = (uint32_t)s->status;
        s_tcb_id[i] = s->flow_id;
    }
    s_nu = nu;
    s_nt = nt;
    g_dirty = 0;
    return RXG_OK;
}

/* ---- registration with the GPU flow tables (g_lock held) ----------------- */
static rxg_udp_sock udp_key(const struct localhost *h) {
    rxg_udp_sock u;
    u.localip = h->localip;
    u.localport = h->localport;
    u.protocol = h->protocol;
    u._pad = 0;
    return u;
}
static rxg_tcb tcb_key(const struct tcp_stream *s) {
    rxg_tcb t;
    t.sip = s->sip;
    t.dip = s->dip;
    t.sport = s->sport;
    t.dport = s->dport;
    t.status = (uint32_t)s->status;
    return t;
}
static int reg_udp(struct localhost *h) { /* LL_ADD (common.c:302) */
    const rxg_udp_sock u = udp_key(h);
    uint32_t id;
    int rc = rxg_flows_add(g_ctx, &u, 1, NULL, 0, &id, NULL);
    if (rc < 0) return rc;
    pthread_mutex_lock(&g_tab);
    uint32_t cap = s_udp_cap;
    if (grow((void **)&s_udp_cb, &s_udp_cap, id + 1, sizeof(void *))) {
        pthread_mutex_unlock(&g_tab);
        return RXG_ENOMEM;
    }
    if (s_udp_cap > cap) memset(s_udp_cb + cap, 0, (s_udp_cap - cap) * sizeof(void *));
    s_udp_cb[id] = h;
    pthread_mutex_unlock(&g_tab);
    h->flow_id = id;
    g_snap_gen++;
    g_dirty = 1;
    return RXG_OK;
}
static int reg_tcb(struct tcp_stream *s) { /* LL_ADD (tcp.c:52, common.c:336) */
    const rxg_tcb t = tcb_key(s);
    uint32_t id;
    int rc = rxg_flows_add(g_ctx, NULL, 0, &t, 1, NULL, &id);
    if (rc < 0) return rc;
    pthread_mutex_lock(&g_tab);
    uint32_t cap = s_tcb_cap;
    if (grow((void **)&s_tcb_cb, &s_tcb_cap, id + 1, sizeof(void *))) {
        pthread_mutex_unlock(&g_tab);
        return RXG_ENOMEM;
    }
    if (s_tcb_cap > cap) memset(s_tcb_cb + cap, 0, (s_tcb_cap - cap) * sizeof(void *));
    s_tcb_cb[id] = s;
    pthread_mutex_unlock(&g_tab);
    s->flow_id = id;
    g_snap_gen++;
    g_dirty = 1;
    return RXG_OK;
}
static void unreg_udp(struct localhost *h) { /* LL_REMOVE (common.c:620) */
    (void)rxg_flows_remove(g_ctx, &h->flow_id, 1, NULL, 0);
    pthread_mutex_lock(&g_tab);
    if (h->flow_id < s_udp_cap) s_udp_cb[h->flow_id] = NULL;
    pthread_mutex_unlock(&g_tab);
    g_snap_gen++;
    g_dirty = 1;
}
static void unreg_tcb(struct tcp_stream *s) { /* LL_REMOVE (tcp.c:321, common.c:660) */
    (void)rxg_flows_remove(g_ctx, NULL, 0, &s->flow_id, 1);
    pthread_mutex_lock(&g_tab);
    if (s->flow_id < s_tcb_cap) s_tcb_cb[s->flow_id] = NULL;
    pthread_mutex_unlock(&g_tab);
    g_snap_gen++;
    g_dirty = 1;
}
static void rekey_udp(struct localhost *h) { /* nbind */
    const rxg_udp_sock u = udp_key(h);
    (void)rxg_flows_update_udp(g_ctx, h->flow_id, &u);
    g_snap_gen++;
    g_dirty = 1;
}
/* key or status of a tcb changed (nbind, nlisten, the state machine); only
 * key and LISTEN changes move lookups (the library ignores the rest) */
static void restate_tcb(struct tcp_stream *s, int lookup_moves) {
    const rxg_tcb t = tcb_key(s);
    (void)rxg_flows_update_tcb(g_ctx, s->flow_id, &t);
    if (lookup_moves) g_snap_gen++;
    g_dirty = 1;
}
/* SYN cookies: the listeners' ids as a bit mask, here and in the library
 * (uploaded ahead of the next submit); after nlisten, the close of a listener
 * and nstack_set_syncookies (g_lock held) */
static int ck_sync_listeners(void) {
    if (!g_ck_mode || !g_ctx) return RXG_OK;
    uint32_t nl = 0, space = 0;
    for (struct tcp_stream *s = g_tcb_set; s; s = s->next)
        if (s->status == TCP_STATUS_LISTEN) {
            nl++;
            if (s->flow_id >= space) space = s->flow_id + 1u;
        }
    uint32_t *ids = malloc((size_t)(nl ? nl : 1) * sizeof(*ids));
    const uint32_t words = (space + 31u) / 32u;
    if (!ids || grow((void **)&s_ck_mask, &s_ck_mask_cap, words ? words : 1, sizeof(uint32_t))) {
        free(ids);
        return RXG_ENOMEM;
    }
    memset(s_ck_mask, 0, (size_t)(words ? words : 1) * sizeof(uint32_t));
    nl = 0;
    for (struct tcp_stream *s = g_tcb_set; s; s = s->next)
        if (s->status == TCP_STATUS_LISTEN) {
            ids[nl++] = s->flow_id;
            s_ck_mask[s->flow_id >> 5] |= 1u << (s->flow_id & 31u);
        }
    g_ck_space = space;
    const int rc = rxg_syncookie_set(g_ctx, &g_ck_p, ids, nl);
    free(ids);
    return rc;
}

/* the GPU TX encoder's state (defined with nstack_tx_burst) */
static int g_tx_encode;
static atomic_ullong g_txe_frames;
static uint32_t g_tx_mss;
static atomic_ullong g_tso_frags;
static uint32_t g_tx_mtu;
static uint16_t g_ip_id;
static atomic_ullong g_udp_frags;
static void tx_stage_free(void);

/* ---- lifecycle ---------------------------------------------------------- */
int nstack_init(int device, uint32_t max_burst, uint64_t max_bytes) {
    pthread_mutex_lock(&g_lock);
    int rc = RXG_OK;
    if (!g_ctx) {
        rc = rxg_open(&g_ctx, device, max_burst, max_bytes);
        if (rc == RXG_OK && g_inplace) rxg_tune_deliver(g_ctx, RXG_DLV_TCP_IN_PLACE);
        if (rc == RXG_OK && g_gro) {
            rxg_tune_deliver(g_ctx, RXG_DLV_TCP_GRO);
            rxg_tune_gro(g_ctx, g_gro);
        }
        if (rc == RXG_OK && (g_order || g_assemble)) rxg_tune_deliver(g_ctx, dlv_flags());
        if (rc == RXG_OK && g_ddos) {
            rxg_tune_deliver(g_ctx, dlv_flags());
            rxg_tune_ddos_thresh(g_ctx, g_ddos_thresh);
        }
        if (rc == RXG_OK && g_ck_mode) {
            rxg_tune_deliver(g_ctx, dlv_flags());
            (void)ck_sync_listeners();
        }
        if (rc == RXG_OK && g_l2) {
            rxg_tune_deliver(g_ctx, dlv_flags());
            (void)l2_sync();
        }
        /* a new context: its delivery sets start again at set 0 */
        for (uint32_t j = 0; j < RXG_DELIVER_DEPTH; j++) g_set_ref[j] = -1;
        g_next_set = 0;
    }
    g_dirty = 1;
    pthread_mutex_unlock(&g_lock);
    return rc;
}

void nstack_fini(void) {
    /* bursts submitted and never completed: waited for, not delivered */
    while (g_pend_n && g_ctx) {
        pend_wait(&g_pend[g_pend_head]);
        g_pend_head = (g_pend_head + 1) % RXG_DELIVER_DEPTH;
        g_pend_n--;
    }
    g_pend_n = g_pend_head = 0;
    for (uint32_t j = 0; j < RXG_DELIVER_DEPTH; j++) {
        free(g_pend[j].v), free(g_pend[j].handled);
        g_pend[j].v = NULL, g_pend[j].handled = NULL;
        g_pend[j].v_cap = g_pend[j].h_cap = 0;
    }
    reclaim();
    pthread_mutex_lock(&g_lock);
    /* unmap every block first (as nclose unregisters before its kill): an
     * application call looks blocks up under g_tab alone, so once the maps
     * are clear no fd_get_ref / drain_all can take a reference on a block the
     * kills below may free */
    pthread_mutex_lock(&g_tab);
    memset(g_fd_cb, 0, sizeof(g_fd_cb));
    free(s_udp_cb), free(s_tcb_cb);
    s_udp_cb = NULL, s_tcb_cb = NULL;
    s_udp_cap = s_tcb_cap = 0;
    pthread_mutex_unlock(&g_tab);
    while (g_pstHost) {
        struct localhost *h = g_pstHost;
        LL_REMOVE(h, g_pstHost);
        udp_kill(h);
    }
    while (g_tcb_set) {
        struct tcp_stream *s = g_tcb_set;
        LL_REMOVE(s, g_tcb_set);
        tcb_kill(s);
    }
    memset(g_ucFdTable, 0, sizeof(g_ucFdTable));
    memset(g_fd_nblk, 0, sizeof(g_fd_nblk));
    free(s_udp), free(s_tcb), free(s_v), free(s_udp_id), free(s_tcb_id), free(s_handled);
    s_udp = NULL, s_tcb = NULL, s_v = NULL, s_udp_id = NULL, s_tcb_id = NULL, s_handled = NULL;
    s_udp_cap = s_tcb_cap = s_v_cap = s_nu = s_nt = s_udp_xcap = s_tcb_xcap = s_handled_cap = 0;
    memset(g_stat, 0, sizeof(g_stat));
    /* every counter nstack_stat reports describes the current stack */
    g_stale_parts = g_copied_bytes = g_pl_waits = 0;
    for (int j = 0; j < 3; j++) atomic_store_explicit(&g_drain_ns[j], 0, memory_order_relaxed);
    atomic_store_explicit(&g_deliveries, 0, memory_order_relaxed);
    bp_drain(); /* (this thread's cached batch blocks; other threads' go when they exit) */
    g_isn_seed = 0;
    while (g_arp) {
        struct arp_entry *e = g_arp;
        LL_REMOVE(e, g_arp);
        free(e);
    }
    g_local_ip = 0;
    memset(g_local_mac, 0, sizeof(g_local_mac));
    reclaim(); /* (what the blocks' last puts let go of) */
    g_inplace = 0; /* (options last one stack) */
    g_gro = 0;
    g_gro_absorbed = 0;
    g_order = 0;
    g_order_moved = 0;
    g_assemble = 0;
    g_asm_dup = g_asm_hole = 0;
    g_ddos = 0;
    g_ddos_thresh = RXG_DDOS_DEFAULT_THRESH;
    memset(&g_ddos_state, 0, sizeof(g_ddos_state));
    memset(&g_ddos_acc, 0, sizeof(g_ddos_acc));
    g_ck_mode = 0;
    g_ck_pin = 0xFFFFFFFFu;
    memset(&g_ck_p, 0, sizeof(g_ck_p));
    g_ck_syn = g_ck_acc = g_ck_rej = 0;
    free(s_ck_mask), free(s_ck_tx), free(s_ck_hst), free(s_ck_htx), free(s_ck_hpk), free(s_ck_hoff);
    free(s_ck_hlen);
    s_ck_mask = NULL, s_ck_tx = NULL, s_ck_hst = NULL, s_ck_htx = NULL, s_ck_hpk = NULL;
    s_ck_hoff = NULL, s_ck_hlen = NULL;
    s_ck_mask_cap = g_ck_space = s_ck_tx_cap = g_ck_tx_head = g_ck_tx_n = s_ck_hcap = 0;
    g_ck_on = 0, g_ck_st = NULL;
    g_l2 = 0;
    g_l2_arp = g_l2_echo = g_l2_drop = g_l2_bad = 0;
    l2_q_clear();
    free(s_l2_one);
    s_l2_one = NULL;
    g_tx_encode = 0;
    atomic_store_explicit(&g_txe_frames, 0, memory_order_relaxed);
    g_tx_mss = 0;
    atomic_store_explicit(&g_tso_frags, 0, memory_order_relaxed);
    g_tx_mtu = 0;
    g_ip_id = 1;
    atomic_store_explicit(&g_udp_frags, 0, memory_order_relaxed);
    tx_stage_free();
    g_mb_release = NULL;
    g_mb_arg = NULL;
    if (g_ctx) rxg_close(g_ctx);
    g_ctx = NULL;
    g_dirty = 1;
    pthread_mutex_unlock(&g_lock);
}

/* ---- socket API (common.c:262-666) --------------------------------------- */
int nsocket(int domain, int type, int protocol) {
    (void)domain, (void)protocol;
    pthread_mutex_lock(&g_lock);
    if (!g_ctx) { /* nstack_init first: the blocks live in its flow tables */
        pthread_mutex_unlock(&g_lock);
        return -1;
    }
    int fd = get_fd_frombitmap();
    if (fd < 0) {
        pthread_mutex_unlock(&g_lock);
        return -1;
    }
    if (type == SOCK_DGRAM) { /* :270-303 */
        struct localhost *h = calloc(1, sizeof(*h));
        if (!h) goto fail;
        h->fd = fd;
        h->protocol = IPPROTO_UDP;
        h->rcvbuf = ring_init(&h->rcv_r, D_RING_SIZE);
        h->sndbuf = ring_init(&h->snd_r, D_RING_SIZE);
        if (!h->rcvbuf || !h->sndbuf) {
            ring_free(h->rcvbuf);
            ring_free(h->sndbuf);
            free(h);
            goto fail;
        }
        pthread_cond_init(&h->cond, NULL);
        pthread_mutex_init(&h->mutex, NULL);
        cb_ref_init(&h->ref);
        if (reg_udp(h)) {
            ring_free(h->rcvbuf);
            ring_free(h->sndbuf);
            free(h);
            goto fail;
        }
        LL_ADD(h, g_pstHost);
        fd_add(fd, h);
    } else if (type == SOCK_STREAM) { /* :304-337 */
        struct tcp_stream *s = calloc(1, sizeof(*s));
        if (!s) goto fail;
        s->fd = fd;
        s->protocol = IPPROTO_TCP;
        s->rcvbuf = ring_init(&s->rcv_r, D_RING_SIZE);
        s->sndbuf = ring_init(&s->snd_r, D_RING_SIZE);
        if (!s->rcvbuf || !s->sndbuf) {
            ring_free(s->rcvbuf);
            ring_free(s->sndbuf);
            free(s);
            goto fail;
        }
        pthread_cond_init(&s->cond, NULL);
        pthread_cond_init(&s->accept_cond, NULL);
        pthread_mutex_init(&s->mutex, NULL);
        cb_ref_init(&s->ref);
        if (reg_tcb(s)) {
            ring_free(s->rcvbuf);
            ring_free(s->sndbuf);
            free(s);
            goto fail;
        }
        LL_ADD(s, g_tcb_set);
        fd_add(fd, s);
    }
    pthread_mutex_unlock(&g_lock);
    return fd;
fail:
    set_fd_frombitmap(fd);
    pthread_mutex_unlock(&g_lock);
    return -1;
}

int nbind(int sockfd, const struct sockaddr *addr, socklen_t addrlen) { /* :342-371 */
    (void)addrlen;
    if (!addr) return -1;
    const struct sockaddr_in *a = (const struct sockaddr_in *)addr;
    pthread_mutex_lock(&g_lock);
    void *info = get_hostinfo_fromfd(sockfd);
    int rc = -1;
    if (info) {
        struct localhost *h = info;
        if (h->protocol == IPPROTO_UDP) {
            h->localport = a->sin_port;
            memcpy(&h->localip, &a->sin_addr.s_addr, 4);
            memcpy(h->localmac, g_local_mac, 6);
            rekey_udp(h);
        } else {
            struct tcp_stream *s = info;
            s->dport = a->sin_port;
            memcpy(&s->dip, &a->sin_addr.s_addr, 4);
            memcpy(s->localmac, g_local_mac, 6);
            s->status = TCP_STATUS_CLOSED;
            restate_tcb(s, 1);
        }
        rc = 0;
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nlisten(int sockfd, int backlog) { /* :373-386 */
    (void)backlog;
    pthread_mutex_lock(&g_lock);
    struct tcp_stream *s = get_hostinfo_fromfd(sockfd);
    int rc = -1;
    if (s) {
        if (s->protocol == IPPROTO_TCP) {
            s->status = TCP_STATUS_LISTEN;
            restate_tcb(s, 1);
            (void)ck_sync_listeners();
        }
        rc = 0;
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int naccept(int sockfd, struct sockaddr *addr, socklen_t *addrlen) { /* :388-416 */
    (void)addrlen;
    pthread_mutex_lock(&g_lock);
    struct tcp_stream *s = get_hostinfo_fromfd(sockfd);
    if (!s || s->protocol != IPPROTO_TCP) {
        pthread_mutex_unlock(&g_lock);
        return -1;
    }
    struct tcp_stream *apt;
    cb_get(&s->ref); /* (the listener may be closed while this call waits) */
    while (!s->dead && (apt = get_accept_tcb(s->dport)) == NULL) {
        /* wait on the listener's cond; g_lock doubles as its mutex here so a
         * tcb added between the check and the wait cannot be missed */
        pthread_cond_wait(&s->accept_cond, &g_lock);
    }
    if (s->dead) {
        tcb_put(s);
        pthread_mutex_unlock(&g_lock);
        errno = EBADF;
        return -1;
    }
    tcb_put(s);
    apt->fd = get_fd_frombitmap();
    fd_add(apt->fd, apt);
    if (addr) {
        struct sockaddr_in *sa = (struct sockaddr_in *)addr;
        sa->sin_family = AF_INET;
        sa->sin_port = apt->sport;
        memcpy(&sa->sin_addr.s_addr, &apt->sip, 4);
    }
    int fd = apt->fd;
    pthread_mutex_unlock(&g_lock);
    return fd;
}

ssize_t nsend(int sockfd, const void *buf, size_t len, int flags) { /* :418-460 */
    (void)flags;
    pthread_mutex_lock(&g_lock);
    struct tcp_stream *s = get_hostinfo_fromfd(sockfd);
    ssize_t n = -1;
    if (s) {
        n = 0;
        if (s->protocol == IPPROTO_TCP) {
            struct tcp_fragment *f = calloc(1, sizeof(*f));
            if (!f) {
                n = -2;
            } else if (!(f->data = calloc(1, len + 1))) {
                free(f);
                n = -1;
            } else {
                f->dport = s->sport;
                f->sport = s->dport;
                f->acknum = s->rcv_nxt;
                f->seqnum = s->snd_nxt;
                f->tcp_flags = 0x10 | 0x08; /* ACK | PSH */
                f->windows = D_TCP_INITIAL_WINDOW;
                f->hdrlen_off = 0x50;
                memcpy(f->data, buf, len);
                f->length = (uint32_t)len;
                pthread_mutex_lock(&s->mutex);
                if (tq_push(s->sndbuf, &s->sq, f)) {
                    free(f->data);
                    free(f);
                    n = -1;
                } else {
                    n = (ssize_t)len;
                }
                pthread_mutex_unlock(&s->mutex);
            }
        }
    }
    pthread_mutex_unlock(&g_lock);
    return n;
}

static ssize_t nrecv_tcb(struct tcp_stream *s, void *buf, size_t len, int flags);

ssize_t nrecv(int sockfd, void *buf, size_t len, int flags) { /* :462-515 */
    struct tcp_stream *s = fd_get_ref(sockfd); /* (linked: the block lives until our put) */
    if (!s) return -1;
    ssize_t r = 0;
    if (s->protocol == IPPROTO_TCP) r = nrecv_tcb(s, buf, len, flags);
    cb_put(s);
    return r;
}

static ssize_t nrecv_tcb(struct tcp_stream *s, void *buf, size_t len, int flags) {
    struct tcp_fragment *f;
    pthread_mutex_lock(&s->mutex);
    while (s->dead || (f = tq_front(s->rcvbuf)) == NULL) {
        if (s->dead) { /* freed (last ACK after nclose) while this call waited */
            pthread_mutex_unlock(&s->mutex);
            errno = EBADF;
            return -1;
        }
        if (flags & MSG_DONTWAIT) {
            pthread_mutex_unlock(&s->mutex);
            errno = EAGAIN;
            return -1;
        }
        pthread_cond_wait(&s->cond, &s->mutex);
    }
    ssize_t length;
    if (f->length > len) { /* :483-496: dequeue, split, re-enqueue the rest at the tail */
        f = tq_detach(s->rcvbuf, &s->rq);
        if (!f) {
            pthread_mutex_unlock(&s->mutex);
            return -1;
        }
        memcpy(buf, f->data, len);
        memmove(f->data, f->data + len, f->length - len);
        f->length -= (uint32_t)len;
        length = f->length; /* the reference returns the REMAINING length here */
        if (tq_push(s->rcvbuf, &s->rq, f)) frag_item_free(f);
    } else { /* :497-514: a 0-length fragment is EOF (returns 0) */
        if (f->length) memcpy(buf, f->data, f->length);
        length = f->length;
        tq_pop(s->rcvbuf, &s->rq);
    }
    pthread_mutex_unlock(&s->mutex);
    return length;
}

static ssize_t udp_recv(struct localhost *h, void *buf, size_t len, int flags,
                        struct sockaddr *src_addr);

ssize_t nrecvfrom(int sockfd, void *buf, size_t len, int flags, struct sockaddr *src_addr,
                  socklen_t *addrlen) { /* :517-565 */
    (void)addrlen;
    struct localhost *h = fd_get_ref(sockfd);
    if (!h) return -1;
    const ssize_t r = udp_recv(h, buf, len, flags, src_addr);
    cb_put(h);
    return r;
}

/* nrecvfrom after the descriptor lookup (common.c:526-565) */
static ssize_t udp_recv(struct localhost *h, void *buf, size_t len, int flags,
                        struct sockaddr *src_addr) {
    struct offload *o = NULL;
    pthread_mutex_lock(&h->mutex);
    while (h->dead || ring_peek(h->rcvbuf, (void **)&o) < 0) {
        if (h->dead) { /* closed by another thread while this call waited */
            pthread_mutex_unlock(&h->mutex);
            errno = EBADF;
            return -1;
        }
        if (flags & MSG_DONTWAIT) {
            pthread_mutex_unlock(&h->mutex);
            errno = EAGAIN;
            return -1;
        }
        pthread_cond_wait(&h->cond, &h->mutex);
    }
    if (o->batch) { /* the next datagram of a batch, read like its own offload */
        struct dgram_batch *b = o->batch;
        const struct dgram_meta *d = &b->meta[b->next++];
        struct offload *spent = NULL; /* the batch, once its last datagram is read */
        if (b->next == b->n) ring_dequeue(h->rcvbuf, (void **)&spent);
        if (src_addr) {
            struct sockaddr_in *a = (struct sockaddr_in *)src_addr;
            a->sin_family = AF_INET;
            a->sin_port = d->sport;
            memcpy(&a->sin_addr.s_addr, &d->sip, 4);
        }
        const uint32_t length = (uint32_t)d->len + 8u; /* offload.length = dgram_len (udp.c:37) */
        if (len < length) { /* :542-556: len bytes out, the rest to the TAIL of the ring */
            struct offload *r = calloc(1, sizeof(*r));
            unsigned char *rest = r ? calloc(1, length - len) : NULL;
            if (rest) {
                if (d->ncopy > len) memcpy(rest, b->data + d->off + len, d->ncopy - len);
                r->sip = d->sip;
                r->sport = d->sport;
                r->protocol = IPPROTO_UDP;
                r->data = rest;
                r->length = (uint16_t)(length - len);
                if (ring_enqueue(h->rcvbuf, r)) offload_free(r), cnt_set(&h->queued, h->queued - 1);
            } else {
                free(r);
                cnt_set(&h->queued, h->queued - 1);
            }
            memset(buf, 0, len);
            memcpy(buf, b->data + d->off, d->ncopy < len ? d->ncopy : len);
            offload_free(spent);
            pthread_mutex_unlock(&h->mutex);
            return (ssize_t)len;
        }
        memcpy(buf, b->data + d->off, d->ncopy); /* :558-564: payload, then zeros */
        memset((unsigned char *)buf + d->ncopy, 0, length - d->ncopy);
        cnt_set(&h->queued, h->queued - 1);
        offload_free(spent);
        pthread_mutex_unlock(&h->mutex);
        return (ssize_t)length;
    }
    ring_dequeue(h->rcvbuf, (void **)&o);
    if (src_addr) {
        struct sockaddr_in *a = (struct sockaddr_in *)src_addr;
        a->sin_family = AF_INET;
        a->sin_port = o->sport;
        memcpy(&a->sin_addr.s_addr, &o->sip, 4);
    }
    if (len < o->length) { /* :542-556: copy len, keep the rest queued */
        memcpy(buf, o->data, len);
        memmove(o->data, o->data + len, o->length - len);
        o->length = (uint16_t)(o->length - len);
        ring_enqueue(h->rcvbuf, o);
        pthread_mutex_unlock(&h->mutex);
        return (ssize_t)len;
    }
    cnt_set(&h->queued, h->queued - 1);
    pthread_mutex_unlock(&h->mutex);
    ssize_t n = o->length; /* :558-564 */
    memcpy(buf, o->data, o->length);
    offload_free(o);
    return n;
}

static ssize_t udp_send(struct localhost *h, const void *buf, size_t len,
                        const struct sockaddr_in *a);

ssize_t nsendto(int sockfd, const void *buf, size_t len, int flags,
                const struct sockaddr *dest_addr, socklen_t addrlen) { /* :567-607 */
    (void)flags, (void)addrlen;
    const struct sockaddr_in *a = (const struct sockaddr_in *)dest_addr;
    if (!a) return -1;
    struct localhost *h = fd_get_ref(sockfd);
    if (!h) return -1;
    const ssize_t r = udp_send(h, buf, len, a);
    cb_put(h);
    return r;
}

/* nsendto after the descriptor lookup (common.c:576-607) */
static ssize_t udp_send(struct localhost *h, const void *buf, size_t len,
                        const struct sockaddr_in *a) {
    struct offload *o = calloc(1, sizeof(*o));
    if (!o) return -1;
    o->dip = a->sin_addr.s_addr;
    o->dport = a->sin_port;
    o->sip = h->localip;
    o->sport = h->localport;
    o->length = (uint16_t)len;
    o->data = malloc(len ? len : 1);
    if (!o->data) {
        free(o);
        return -1;
    }
    memcpy(o->data, buf, len);
    pthread_mutex_lock(&h->mutex);
    int e = ring_enqueue(h->sndbuf, o);
    pthread_mutex_unlock(&h->mutex);
    if (e) {
        free(o->data);
        free(o);
        return -1;
    }
    return (ssize_t)len;
}

int nclose(int fd) { /* :609-666 */
    pthread_mutex_lock(&g_lock);
    void *info = get_hostinfo_fromfd(fd);
    if (!info) {
        pthread_mutex_unlock(&g_lock);
        return -1;
    }
    struct localhost *h = info;
    if (h->protocol == IPPROTO_UDP) {
        unreg_udp(h);
        LL_REMOVE(h, g_pstHost);
        fd_del(fd, h);
        udp_kill(h); /* (freed now, or by the last reader's put) */
        set_fd_frombitmap(fd);
    } else {
        struct tcp_stream *s = info;
        if (s->status != TCP_STATUS_LISTEN) { /* queue FIN, wait for LAST_ACK */
            struct tcp_fragment *f = calloc(1, sizeof(*f));
            if (f) {
                f->sport = s->dport;
                f->dport = s->sport;
                f->seqnum = s->snd_nxt;
                f->acknum = s->rcv_nxt;
                f->tcp_flags = 0x01 | 0x10; /* FIN | ACK */
                f->windows = D_TCP_INITIAL_WINDOW;
                f->hdrlen_off = 0x50;
                pthread_mutex_lock(&s->mutex);
                if (tq_push(s->sndbuf, &s->sq, f)) free(f);
                pthread_mutex_unlock(&s->mutex);
            }
            s->status = TCP_STATUS_LAST_ACK;
            restate_tcb(s, 0);
            set_fd_frombitmap(fd);
        } else {
            unreg_tcb(s);
            LL_REMOVE(s, g_tcb_set);
            fd_del(fd, s);
            tcb_kill(s);
            (void)ck_sync_listeners();
            /* the reference leaves the listener's fd set in the bitmap here */
        }
    }
    pthread_mutex_unlock(&g_lock);
    return 0;
}

/* ---- receive path --------------------------------------------------------- */
static inline uint32_t rd32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
static inline uint16_t rd16(const uint8_t *p) {
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}

static inline uint32_t rdbe32(const uint8_t *p) { return ntohl(rd32(p)); }

/* ---- TCP state machine (tcp.c:3-331, dispatch :373-415), driven by verdicts.
 * Where tcp.c holds unresolved merge-conflict hunks the HEAD side is taken
 * (rcv_nxt += payloadlen at :244-248 and :266-279, no ntohl round trip). */

/* tcp_stream_search (common.c:31-55) over the live list: the exact 4-tuple
 * (status ignored), else the first LISTEN block on dport (dst IP ignored).
 * Answered in O(1) by the context's host image of the flow tables, which
 * every block change updates at once (reg_tcb / unreg_tcb / restate_tcb:
 * newest-first chains per key, the newest LISTEN block per port), instead of
 * the reference's two list walks (~192 us each at 64K tcbs). */
static struct tcp_stream *tcb_search(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport) {
    const uint32_t id = rxg_ft_lookup_tcp(g_ctx, sip, dip, sport, dport);
    return id < s_tcb_cap ? s_tcb_cb[id] : NULL;
}

static struct tcp_stream *tcb_new(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport,
                                  int status) { /* tcp_stream_create, tcp.c:3-41 */
    struct tcp_stream *s = calloc(1, sizeof(*s));
    if (!s) return NULL;
    s->sip = sip;
    s->dip = dip;
    s->sport = sport;
    s->dport = dport;
    s->protocol = IPPROTO_TCP;
    s->fd = -1;
    s->status = status;
    s->rcvbuf = ring_init(&s->rcv_r, D_RING_SIZE);
    s->sndbuf = ring_init(&s->snd_r, D_RING_SIZE);
    if (!s->rcvbuf || !s->sndbuf) {
        ring_free(s->rcvbuf);
        ring_free(s->sndbuf);
        free(s);
        return NULL;
    }
    memcpy(s->localmac, g_local_mac, 6); /* tcp.c:32 */
    if (!g_isn_seed) g_isn_seed = (unsigned int)time(NULL);
    s->snd_nxt = (uint32_t)((unsigned long)rand_r(&g_isn_seed) % D_TCP_MAX_SEQ);
    pthread_cond_init(&s->cond, NULL);
    pthread_cond_init(&s->accept_cond, NULL);
    pthread_mutex_init(&s->mutex, NULL);
    cb_ref_init(&s->ref);
    return s;
}

/* tcp.c:107-116: the listener tcp_stream_search(0, 0, 0, dport) finds is
 * woken (its naccept) */
static void wake_acceptors(uint16_t dport) {
    struct tcp_stream *l = tcb_search(0, 0, 0, dport);
    if (l) pthread_cond_broadcast(&l->accept_cond);
}

static void queue_ctl(struct tcp_stream *s, uint16_t sport_raw, uint16_t dport_raw, uint8_t flags) {
    struct tcp_fragment *f = calloc(1, sizeof(*f)); /* ng_tcp_send_ackpkt, tcp.c:187-216 */
    if (!f) return;
    f->sport = sport_raw;
    f->dport = dport_raw;
    f->seqnum = s->snd_nxt;
    f->acknum = s->rcv_nxt;
    f->tcp_flags = flags;
    f->windows = D_TCP_INITIAL_WINDOW;
    f->hdrlen_off = 0x50;
    pthread_mutex_lock(&s->mutex);
    if (tq_push(s->sndbuf, &s->sq, f)) free(f);
    pthread_mutex_unlock(&s->mutex);
}

/* ng_tcp_enqueue_recvbuffer, tcp.c:133-185: payloadlen = tcplen - 4*hl;
 * > 0: a copy of the payload (bytes past the capture read as 0), 0 or < 0: a
 * 0-length fragment (nrecv's EOF) */
static void tcp_enqueue_rcv(struct tcp_stream *s, const uint8_t *f, uint32_t cap, int tcplen) {
    struct tcp_fragment *fr = calloc(1, sizeof(*fr));
    if (!fr) return;
    const uint32_t hl = (cap > 46 ? f[46] : 0) >> 4;
    fr->dport = ntohs(cap >= 38 ? rd16(f + 36) : 0);
    fr->sport = ntohs(cap >= 36 ? rd16(f + 34) : 0);
    const int plen = tcplen - (int)hl * 4;
    if (plen > 0) {
        fr->data = malloc((size_t)plen + 1);
        if (!fr->data) {
            free(fr);
            return;
        }
        const uint32_t from = 34 + hl * 4;
        const uint32_t avail = cap > from ? cap - from : 0;
        const uint32_t ncopy = (uint32_t)plen < avail ? (uint32_t)plen : avail;
        memcpy(fr->data, f + from, ncopy);
        memset(fr->data + ncopy, 0, (size_t)plen + 1 - ncopy); /* past the capture, and a NUL */
        fr->length = (uint32_t)plen;
    }
    pthread_mutex_lock(&s->mutex);
    int e = tq_push(s->rcvbuf, &s->rq, fr);
    if (!e) pthread_cond_signal(&s->cond);
    pthread_mutex_unlock(&s->mutex);
    if (e) {
        free(fr->data);
        free(fr);
        g_stat[1]++;
    } else {
        g_stat[4]++;
    }
}

/* Stream assembly on, one frame of an ESTABLISHED connection on the
 * frame-by-frame path: the host rule of rxgpu.h ("TCP stream assembly") on a
 * stream of one (seq, bytes = the payload when it was captured whole, with or
 * without PSH; FIN when the frame was usable).  Bytes below rcv_nxt are passed
 * over, a frame behind a hole only draws an ACK. */
static void tcp_dispatch_assembled(struct tcp_stream *s, const uint8_t *f, uint32_t cap, int tcplen,
                                   uint8_t fl, uint16_t sport, uint16_t dport, uint32_t seq,
                                   uint32_t ack) {
    if (fl & 0x06u) return; /* (SYN or RST: left alone, no bytes, no FIN) */
    const uint32_t hl = (cap > 46 ? f[46] : 0) >> 4;
    const int plen = tcplen - (int)hl * 4;
    const uint32_t from = 34 + hl * 4, avail = cap > from ? cap - from : 0;
    const int usable = plen <= 0 || avail >= (uint32_t)plen;
    const uint32_t bytes = plen > 0 && usable ? (uint32_t)plen : 0;
    const int fin = (fl & TCP_FIN) && usable;
    if (!bytes && !fin) return; /* (a pure ACK) */
    const int32_t d = (int32_t)(s->rcv_nxt - seq);
    if (d < 0) { /* behind a hole */
        g_asm_hole++;
        queue_ctl(s, dport, sport, TCP_ACK);
        return;
    }
    const uint32_t fresh = bytes > (uint32_t)d ? bytes - (uint32_t)d : 0;
    g_asm_dup += bytes - fresh;
    if (fresh) {
        struct tcp_fragment *fr = calloc(1, sizeof(*fr));
        if (fr) fr->data = malloc((size_t)fresh + 1);
        if (fr && fr->data) {
            fr->dport = ntohs(dport);
            fr->sport = ntohs(sport);
            memcpy(fr->data, f + from + (uint32_t)d, fresh);
            fr->data[fresh] = 0;
            fr->length = fresh;
            pthread_mutex_lock(&s->mutex);
            int e = tq_push(s->rcvbuf, &s->rq, fr);
            if (!e) pthread_cond_signal(&s->cond);
            pthread_mutex_unlock(&s->mutex);
            if (e) {
                free(fr->data);
                free(fr);
                g_stat[1]++;
            } else {
                g_stat[4]++;
            }
        } else {
            free(fr);
        }
        s->rcv_nxt += fresh;
    }
    if (fin && (uint32_t)d <= bytes) {
        s->status = TCP_STATUS_CLOSE_WAIT;
        restate_tcb(s, 0);
        tcp_enqueue_rcv(s, f, cap, (int)hl * 4); /* EOF marker (payloadlen 0) */
        s->rcv_nxt += 1;
    }
    s->snd_nxt = ack;
    queue_ctl(s, dport, sport, TCP_ACK);
}

/* tcp_process after the lookup (tcp.c:373-415) for the frame's tcb (g_lock held) */
static void tcp_dispatch(struct tcp_stream *s, const uint8_t *f, uint32_t cap);
static void tcp_dispatch(struct tcp_stream *s, const uint8_t *f, uint32_t cap) {
    const uint8_t fl = cap > 47 ? f[47] : 0;
    const uint16_t sport = cap >= 36 ? rd16(f + 34) : 0, dport = cap >= 38 ? rd16(f + 36) : 0;
    const uint32_t seq = cap >= 42 ? rdbe32(f + 38) : 0, ack = cap >= 46 ? rdbe32(f + 42) : 0;
    switch (s->status) {
    case TCP_STATUS_LISTEN: /* tcp_handle_listen, tcp.c:43-87 */
        if (g_ck_on) { /* SYN cookies: no tcb from any SYN; one from a verified ACK */
            uint8_t st = g_ck_cur;
            g_ck_cur = 0; /* (the frame dispatched again below is not a listener's) */
            if (st == CK_JUDGE) {
                rxg_txd d;
                st = ck_judge_frame(f, cap, &d);
                if (st == RXG_CK_SYN) ck_tx_push(&d, 1), g_ck_syn++;
                if (st == RXG_CK_ACK_BAD) g_ck_rej++;
            }
            if (st != RXG_CK_ACK_OK) break;
            struct tcp_stream *c = tcb_new(rd32(f + 26), rd32(f + 30), sport, dport, TCP_STATUS_ESTABLISHED);
            if (!c) return;
            c->rcv_nxt = seq, c->snd_nxt = ack; /* (the client's isn + 1, the cookie + 1) */
            if (reg_tcb(c)) {
                ring_free(c->rcvbuf);
                ring_free(c->sndbuf);
                free(c);
                return;
            }
            LL_ADD(c, g_tcb_set);
            g_burst_mutated = 1;
            g_ck_acc++;
            wake_acceptors(c->dport);
            tcp_dispatch(c, f, cap); /* piggybacked data or a FIN: the ESTABLISHED path */
            break;
        }
        if (fl & TCP_SYN) {
            struct tcp_stream *syn = tcb_new(cap >= 30 ? rd32(f + 26) : 0, cap >= 34 ? rd32(f + 30) : 0,
                                             sport, dport, TCP_STATUS_LISTEN);
            if (!syn) return;
            /* registered as it ends this handler: SYN_RCVD (the LISTEN of
             * tcp_stream_create is overwritten before any other lookup) */
            syn->status = TCP_STATUS_SYN_RCVD;
            if (reg_tcb(syn)) {
                ring_free(syn->rcvbuf);
                ring_free(syn->sndbuf);
                free(syn);
                return;
            }
            LL_ADD(syn, g_tcb_set);
            g_burst_mutated = 1;
            syn->rcv_nxt = seq + 1;
            queue_ctl(syn, dport, sport, TCP_SYN | TCP_ACK);
        }
        break;
    case TCP_STATUS_SYN_RCVD: /* tcp_handle_syn_rcvd, tcp.c:89-131 */
        if (fl & TCP_ACK) {
            s->status = TCP_STATUS_ESTABLISHED; /* acknum == snd_nxt + 1 only printed */
            restate_tcb(s, 0);
            wake_acceptors(s->dport);
        }
        break;
    case TCP_STATUS_ESTABLISHED: { /* tcp_handle_established, tcp.c:218-297 */
        const int tcplen = (int)(cap >= 18 ? ((uint32_t)f[16] << 8 | f[17]) : 0) - 20; /* :391 */
        if (g_assemble) { /* the frame as a stream of one, aligned with rcv_nxt */
            tcp_dispatch_assembled(s, f, cap, tcplen, fl, sport, dport, seq, ack);
            break;
        }
        if (fl & TCP_PSH) {
            tcp_enqueue_rcv(s, f, cap, tcplen);
            const int plen = tcplen - (int)((cap > 46 ? f[46] : 0) >> 4) * 4;
            s->rcv_nxt = s->rcv_nxt + (uint32_t)plen;
            s->snd_nxt = ack;
            queue_ctl(s, dport, sport, TCP_ACK);
        }
        if (fl & TCP_FIN) {
            s->status = TCP_STATUS_CLOSE_WAIT;
            restate_tcb(s, 0);
            tcp_enqueue_rcv(s, f, cap, (cap > 46 ? f[46] : 0) >> 4); /* EOF marker */
            s->rcv_nxt = s->rcv_nxt + 1;
            s->snd_nxt = ack;
            queue_ctl(s, dport, sport, TCP_ACK);
        }
        break;
    }
    case TCP_STATUS_LAST_ACK: /* tcp_handle_last_ack, tcp.c:312-331 */
        if (fl & TCP_ACK) {
            s->status = TCP_STATUS_CLOSED;
            unreg_tcb(s);
            LL_REMOVE(s, g_tcb_set);
            fd_del(s->fd, s);
            tcb_kill(s); /* (a reader blocked in nrecv wakes and returns) */
            g_burst_mutated = 1;
        }
        break;
    default: /* CLOSED, SYN_SENT, FIN_WAIT_*, CLOSING, TIME_WAIT, CLOSE_WAIT: no-ops */
        break;
    }
}

/* one TCP verdict (g_lock held).  The verdict's lookup is the one the
 * reference would make against the snapshot the burst was classified with;
 * once this burst's own deliveries have changed the tcb list (a SYN created
 * a tcb, an ACK in LAST_ACK freed one), later segments are looked up again on
 * the live list, as the reference's frame-by-frame loop would.  Returns the
 * reference's rc for the frame. */
static int deliver_tcp(const rxg_mbuf *m, const rxg_verdict *v, uint8_t ckst) {
    if (v->rc == RXG_RC_TCP_BAD_CKSUM) return v->rc; /* depends on the bytes only */
    const uint8_t *f = (const uint8_t *)m->buf_addr + m->data_off;
    const uint32_t cap = m->data_len;
    struct tcp_stream *s;
    if (g_burst_mutated || g_burst_stale)
        s = tcb_search(cap >= 30 ? rd32(f + 26) : 0, cap >= 34 ? rd32(f + 30) : 0,
                       cap >= 36 ? rd16(f + 34) : 0, cap >= 38 ? rd16(f + 36) : 0);
    else
        s = (v->rc == RXG_RC_OK && v->flow_id < s_tcb_cap) ? s_tcb_cb[v->flow_id] : NULL;
    if (!s) return RXG_RC_TCP_NO_TCB;
    g_stat[2]++;
    /* the burst's status holds for the block the verdict named */
    g_ck_cur = ckst != CK_JUDGE && v->rc == RXG_RC_OK && v->flow_id < s_tcb_cap &&
                       s_tcb_cb[v->flow_id] == s
                   ? ckst
                   : CK_JUDGE;
    tcp_dispatch(s, f, cap);
    return RXG_RC_OK;
}

/* get_hostinfo_fromip_port (common.c:97-108) over the live list, answered
 * by the host image of the flow tables (O(1), as tcb_search) */
static struct localhost *udp_search(uint32_t dip, uint16_t dport) {
    const uint32_t id = rxg_ft_lookup_udp(g_ctx, dip, dport);
    return id < s_udp_cap ? s_udp_cb[id] : NULL;
}

/* udp.c:25-52 for one verdict (g_lock held).  A verdict made for an older
 * snapshot (g_burst_stale) is looked up again on the live list: its flow id
 * may name another socket once one has been closed. */
static int deliver_one(const rxg_mbuf *m, const rxg_verdict *v, int *rc) {
    if (v->cls == RXG_CLS_TCP) return 0;
    if (v->cls != RXG_CLS_UDP) {
        g_stat[3]++;
        return 0;
    }
    if (g_udp_done) return 0;
    const uint8_t *f = (const uint8_t *)m->buf_addr + m->data_off;
    const uint32_t cap = m->data_len;
    struct localhost *h;
    if (g_burst_stale) {
        h = udp_search(cap >= 34 ? rd32(f + 30) : 0, cap >= 38 ? rd16(f + 36) : 0);
        *rc = !h ? RXG_RC_UDP_NO_SOCKET
                 : ((v->flags & RXG_F_UDP_SHORT) ? RXG_RC_UDP_NOMEM : RXG_RC_OK);
        if (*rc != RXG_RC_OK) return 0;
    } else {
        if (v->rc != RXG_RC_OK || v->flow_id >= s_udp_cap || !s_udp_cb[v->flow_id]) return 0;
        h = s_udp_cb[v->flow_id];
    }
    struct offload *o = calloc(1, sizeof(*o));
    if (!o) return 0;
    o->sip = cap >= 30 ? rd32(f + 26) : 0;
    o->dip = cap >= 34 ? rd32(f + 30) : 0;
    o->sport = cap >= 36 ? rd16(f + 34) : 0;
    o->dport = cap >= 38 ? rd16(f + 36) : 0;
    o->protocol = IPPROTO_UDP;
    o->length = (uint16_t)(v->payload_len + 8); /* = dgram_len (udp.c:37) */
    o->data = calloc(1, o->length);             /* payload + 8 zero bytes (see nstack.h) */
    if (!o->data) {
        free(o);
        return 0;
    }
    uint32_t avail = cap > v->payload_off ? cap - v->payload_off : 0;
    uint32_t ncopy = v->payload_len < avail ? v->payload_len : avail;
    memcpy(o->data, f + v->payload_off, ncopy); /* udp.c:46 */
    pthread_mutex_lock(&h->mutex);
    int e = h->queued >= D_RING_SIZE ? -ENOBUFS : ring_enqueue(h->rcvbuf, o); /* udp.c:48 */
    if (!e) cnt_set(&h->queued, h->queued + 1), pthread_cond_signal(&h->cond); /* udp.c:50-52 */
    pthread_mutex_unlock(&h->mutex);
    if (e) {
        free(o->data);
        free(o);
        g_stat[1]++;
        return 0;
    }
    g_stat[0]++;
    return 1;
}

static const uint8_t *arp_lookup(uint32_t ip) { /* ng_get_dst_macaddr, common.c:161-175 */
    for (struct arp_entry *e = g_arp; e; e = e->next)
        if (e->ip == ip) return e->mac;
    return NULL;
}

static int arp_insert(uint32_t ip, const uint8_t *mac) { /* ng_arp_entry_insert, common.c:177-204 */
    if (arp_lookup(ip)) return 0;
    struct arp_entry *e = calloc(1, sizeof(*e));
    if (!e) return 0;
    e->ip = ip;
    memcpy(e->mac, mac, 6);
    LL_ADD(e, g_arp);
    return 1;
}

/* the ARP branch of pkt_process (netfamily.c:156-170): an ARP frame whose
 * target protocol address is the local IP teaches (sender, Ethernet source).
 * The reference inserts pstIpHdr->src_addr there, a pointer left over from an
 * earlier IPv4 frame (uninitialised before the first); the ARP sender
 * protocol address is what that code means and is used here. */
static void arp_learn(const rxg_mbuf *m) {
    const uint8_t *f = (const uint8_t *)m->buf_addr + m->data_off;
    if (m->data_len < 42 || rd32(f + 38) != g_local_ip) return;
    arp_insert(rd32(f + 28), f + 6);
}

/* verdicts -> sockets, frame by frame in burst order (g_lock held); frames
 * marked in `handled` (nullable) were delivered already (deliver_tcp_sorted) */
static int deliver_burst(rxg_mbuf *const *m, uint32_t n, const rxg_verdict *v, int *rc_out,
                         const uint8_t *handled) {
    int delivered = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (handled && handled[i]) continue;
        int rc = v[i].rc;
        if (v[i].cls == RXG_CLS_ARP) arp_learn(m[i]);
        if (v[i].cls == RXG_CLS_TCP)
            rc = deliver_tcp(m[i], &v[i], g_ck_st ? g_ck_st[i] : CK_JUDGE);
        else
            delivered += deliver_one(m[i], &v[i], &rc);
        if (rc_out) rc_out[i] = rc;
    }
    g_burst_stale = 0;
    return delivered;
}

/* the bytes of a datagram's len payload bytes the frame's capture holds
 * (min(dgram_len - 8, caplen - 42)) */
static inline uint32_t dgram_captured(const rxg_mbuf *mb, uint32_t len) {
    const uint32_t avail = mb->data_len > 42u ? mb->data_len - 42u : 0u;
    return len < avail ? len : avail;
}

/* The datagram records of a burst whose verdicts came from elsewhere
 * (nstack_deliver), as the GPU's compaction hands them to nstack_rx_burst
 * (rxg_udp_compact_dev): the rc-0 UDP verdicts naming a live socket id,
 * grouped by id in burst order (first[f] .. first[f + 1]), each captured
 * payload (dgram_captured) at a 16-B aligned offset of one buffer, a socket's
 * payloads contiguous.  So the host-only path delivers UDP through the same
 * batches.  Returns the datagrams (0: none, or out of memory: the
 * frame-by-frame path then delivers them); *payload is the buffer to free. */
static uint32_t host_dgrams(rxg_mbuf *const *m, uint32_t n, const rxg_verdict *v, uint32_t nf,
                            rxg_dgram **dg_out, uint32_t **first_out, uint8_t **payload) {
    *dg_out = NULL, *first_out = NULL, *payload = NULL;
    uint32_t *first = calloc((size_t)nf + 2, sizeof(uint32_t));
    if (!first) return 0;
    uint32_t nd = 0;
    for (uint32_t i = 0; i < n; i++)
        if (v[i].cls == RXG_CLS_UDP && v[i].rc == RXG_RC_OK && v[i].flow_id < nf &&
            s_udp_cb[v[i].flow_id])
            first[v[i].flow_id + 1]++, nd++;
    rxg_dgram *dg = nd ? malloc((size_t)nd * sizeof(*dg)) : NULL;
    uint32_t *pos = nd ? malloc((size_t)nf * sizeof(uint32_t)) : NULL;
    if (!dg || !pos) {
        free(first), free(dg), free(pos);
        return 0;
    }
    for (uint32_t f = 0; f < nf; f++) first[f + 1] += first[f], pos[f] = first[f];
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!(v[i].cls == RXG_CLS_UDP && v[i].rc == RXG_RC_OK && v[i].flow_id < nf &&
              s_udp_cb[v[i].flow_id]))
            continue;
        const uint8_t *f = (const uint8_t *)m[i]->buf_addr + m[i]->data_off;
        const uint32_t cap = m[i]->data_len;
        rxg_dgram *d = &dg[pos[v[i].flow_id]++];
        d->frame = i;
        d->sip = cap >= 30 ? rd32(f + 26) : 0;
        d->sport = cap >= 36 ? rd16(f + 34) : 0;
        d->len = (uint16_t)v[i].payload_len;
        bytes += (dgram_captured(m[i], d->len) + 15u) & ~15u;
    }
    free(pos);
    uint8_t *pl = malloc(bytes + 16);
    if (!pl) {
        free(first), free(dg);
        return 0;
    }
    uint32_t off = 0;
    for (uint32_t j = 0; j < nd; j++) { /* socket by socket: each one's payloads contiguous */
        rxg_dgram *d = &dg[j];
        const rxg_mbuf *mb = m[d->frame];
        const uint32_t c = dgram_captured(mb, d->len);
        d->offset = off;
        memcpy(pl + off, (const uint8_t *)mb->buf_addr + mb->data_off + 42u, c);
        off += (c + 15u) & ~15u;
    }
    *dg_out = dg, *first_out = first, *payload = pl;
    return nd;
}

/* UDP delivery of a whole burst from the GPU's compaction (g_lock held):
 * socket by socket, its datagrams (burst order) in one batch item, their
 * captured payloads in one memcpy; a full ring keeps the first datagrams and
 * drops the rest, as successive enqueues would (udp.c:48) */
static int deliver_udp_batches(rxg_mbuf *const *m, const rxg_dgram *dg, const uint32_t *first,
                               const uint8_t *payload, uint32_t nf) {
    int delivered = 0;
    for (uint32_t f = 0; f < nf; f++) {
        const uint32_t a = first[f], k = first[f + 1] - a;
        if (!k) continue;
        struct localhost *h = f < s_udp_cap ? s_udp_cb[f] : NULL;
        if (!h) continue; /* (not reached: verdicts name live sockets) */
        pthread_mutex_lock(&h->mutex);
        const uint32_t room = h->queued < D_RING_SIZE ? D_RING_SIZE - h->queued : 0;
        const uint32_t take = k < room ? k : room;
        g_stat[1] += k - take;
        if (!take) {
            pthread_mutex_unlock(&h->mutex);
            continue;
        }
        const rxg_dgram *d0 = &dg[a], *dl = &dg[a + take - 1];
        const size_t bytes =
            (size_t)(dl->offset - d0->offset) + dgram_captured(m[dl->frame], dl->len);
        struct offload *o = bp_alloc(sizeof(*o) + sizeof(struct dgram_batch) +
                                     take * sizeof(struct dgram_meta) + bytes + 1);
        if (!o) {
            g_stat[1] += take;
            pthread_mutex_unlock(&h->mutex);
            continue;
        }
        memset(o, 0, sizeof(*o));
        struct dgram_batch *b = (struct dgram_batch *)(o + 1);
        b->n = take;
        b->next = 0;
        b->meta = (struct dgram_meta *)(b + 1);
        b->data = (unsigned char *)(b->meta + take);
        memcpy(b->data, payload + d0->offset, bytes); /* the socket's slice, once */
        for (uint32_t j = 0; j < take; j++) {
            const rxg_dgram *d = &dg[a + j];
            b->meta[j].sip = d->sip;
            b->meta[j].sport = d->sport;
            b->meta[j].len = d->len;
            b->meta[j].ncopy = (uint16_t)dgram_captured(m[d->frame], d->len);
            b->meta[j].off = d->offset - d0->offset;
        }
        o->batch = b;
        o->protocol = IPPROTO_UDP;
        if (ring_enqueue(h->rcvbuf, o)) { /* (the item ring holds >= D_RING_SIZE) */
            offload_free(o);
            g_stat[1] += take;
        } else {
            cnt_set(&h->queued, h->queued + take);
            g_stat[0] += take;
            delivered += (int)take;
            pthread_cond_signal(&h->cond); /* udp.c:50-52 */
        }
        pthread_mutex_unlock(&h->mutex);
    }
    return delivered;
}

/* ---- TCP delivery of a burst, connection by connection ---------------------
 * A connection's segments of one burst, from the GPU's segment sort, through
 * tcp_handle_established (tcp.c:218-297) in burst order (g_lock held).  Only
 * for a tcb whose state cannot move a lookup: ESTABLISHED (it may go to
 * CLOSE_WAIT on a FIN, which no lookup reads) and the states whose segments
 * are no-ops (CLOSE_WAIT, CLOSED, ...).  Such a tcb's segments interact with
 * no other frame of the burst (no block is created or freed for them, and
 * every frame of their 4-tuple names this tcb), so running them connection
 * by connection equals the reference's frame-by-frame loop.  The receive
 * fragments the segments queue (ng_tcp_enqueue_recvbuffer, tcp.c:133-185)
 * and the ACKs they send (tcp.c:187-216) go in as one batch item each: one
 * allocation.  Both connection functions below work in the same four steps:
 * count what the records make, open the pair of batches (conn_open), walk the
 * records writing fragments (put_frag) and ACKs (put_ack), close (conn_close).
 * The steps are always inlined (CONN_STEP), as the hand-written copies they
 * replace were: at 4 segments per connection a call per step shows in phase 7,
 * and put_frag out of line cost in-place delivery 5 %
 * (profiles/nstack_deliver_refactor/sock_ab.txt). */
#define CONN_STEP static inline __attribute__((always_inline))
struct conn_batch {
    struct frag_batch *rb, *ab; /* receive fragments, ACKs (NULL: no room, or out of memory) */
    uint32_t rtake, atake;      /* the fragments the rings have room for */
    unsigned char *pp;          /* where the next copied payload goes in rb's block */
    uint32_t fi, ai;            /* fragments / ACKs made so far (those past the room too) */
};

/* The connection takes its k records (marked in handled, rc 0, stat 2), or
 * returns 1: its state needs the frame-by-frame path (LISTEN, SYN_RCVD,
 * LAST_ACK: tcp_dispatch validates each frame there) */
CONN_STEP int conn_claim(const struct tcp_stream *s, const rxg_segment *sg, uint32_t k,
                      uint8_t *handled, int *rc_out) {
    if (s->status == TCP_STATUS_LISTEN || s->status == TCP_STATUS_SYN_RCVD ||
        s->status == TCP_STATUS_LAST_ACK)
        return 1;
    for (uint32_t j = 0; j < k; j++) {
        handled[sg[j].frame] = 1;
        if (rc_out) rc_out[sg[j].frame] = RXG_RC_OK;
    }
    g_stat[2] += k;
    return 0;
}

CONN_STEP struct frag_batch *frag_batch_new(uint32_t n, uint64_t extra) {
    struct frag_batch *b = bp_alloc(sizeof(*b) + n * sizeof(struct tcp_fragment) + extra);
    if (!b) return NULL;
    memset(&b->item, 0, sizeof(b->item));
    b->item.batch = b;
    b->n = n;
    b->next = 0;
    b->frag = (struct tcp_fragment *)(b + 1);
    b->pl_ref = -1;
    return b;
}

/* s->mutex taken (conn_close lets it go); room for nfr fragments with pbytes
 * of copied payload and nack ACKs: only those that fit (a full ring drops the
 * rest, as successive enqueues would) */
CONN_STEP void conn_open(struct conn_batch *cb, struct tcp_stream *s, uint32_t nfr, uint32_t nack,
                      uint64_t pbytes) {
    pthread_mutex_lock(&s->mutex);
    const uint32_t rroom = s->rq < D_RING_SIZE ? D_RING_SIZE - s->rq : 0;
    const uint32_t aroom = s->sq < D_RING_SIZE ? D_RING_SIZE - s->sq : 0;
    cb->rtake = nfr < rroom ? nfr : rroom, cb->atake = nack < aroom ? nack : aroom;
    cb->rb = cb->rtake ? frag_batch_new(cb->rtake, pbytes + 1) : NULL;
    cb->ab = cb->atake ? frag_batch_new(cb->atake, 0) : NULL;
    cb->pp = cb->rb ? (unsigned char *)(cb->rb->frag + cb->rtake) : NULL;
    cb->fi = cb->ai = 0;
}

/* the two batches onto the tcb's rings, the reader woken, s->mutex let go */
CONN_STEP void conn_close(struct conn_batch *cb, struct tcp_stream *s) {
    struct frag_batch *rb = cb->rb, *ab = cb->ab;
    if (rb) {
        if (rb->pl_ref >= 0) { /* until the batch is freed */
            rxg_payload_hold(g_ctx, rb->pl_ref);
            atomic_fetch_add_explicit(&g_pl_batches, 1, memory_order_relaxed);
            atomic_fetch_add_explicit(&g_pl_out[rb->pl_ref], 1, memory_order_relaxed);
        }
        if (ring_enqueue(s->rcvbuf, &rb->item)) { /* (not reached: items <= fragments <= capacity) */
            frag_item_free(&rb->item);
            g_stat[4] -= cb->rtake, g_stat[1] += cb->rtake;
        } else {
            cnt_set(&s->rq, s->rq + cb->rtake);
            pthread_cond_signal(&s->cond); /* tcp.c:178-180 */
        }
    }
    if (ab) {
        if (ring_enqueue(s->sndbuf, &ab->item))
            bp_free(ab);
        else
            cnt_set(&s->sq, s->sq + cb->atake);
    }
    pthread_mutex_unlock(&s->mutex);
}

/* a segment's payload in its frame */
static inline unsigned char *seg_payload(rxg_mbuf *const *m, const rxg_segment *g) {
    const rxg_mbuf *mb = m[g->frame];
    return (unsigned char *)mb->buf_addr + mb->data_off + 34u + 4u * g->hl;
}

/* The bytes of one receive fragment: `length` of them (0: the 0-length EOF
 * fragment), the first ncopy captured (what is past them reads 0), carried by
 * the records g[0..nseg) — in their frames, and from `offset` of the burst's
 * payload buffer when the library gathered one.  tail: each record holds the
 * last ncopy bytes of its payload (assembly: ncopy = take) and the fragment
 * starts `skip` bytes into them; otherwise the first ncopy, skip = 0. */
struct frag_src {
    const rxg_segment *g;
    uint32_t nseg, offset, length, ncopy, skip;
    int tail;
};

/* One receive fragment (tcp.c:133-185), ports from x->g; g_stat as
 * tcp_enqueue_rcv (4: queued, 1: no room).  Bytes captured whole stay where
 * they are — in the frame with its mbuf held (inpl; one record), or in the
 * held pooled buffer pl_ref — and the batch keeps them until it is freed;
 * otherwise they are copied into the batch's block, from the payload buffer
 * or (host verdicts: payload NULL) gathered from the frames, zero filled past
 * the capture.  Each caller's constants (one record, no in-place, the EOF's
 * length 0) leave it the branches that caller can take. */
CONN_STEP void put_frag(struct conn_batch *cb, const struct frag_src *x, const uint8_t *payload,
                        int32_t pl_ref, rxg_mbuf *const *m, int inpl) {
    if (cb->fi++ >= cb->rtake || !cb->rb) {
        g_stat[1]++;
        return;
    }
    struct tcp_fragment *fr = &cb->rb->frag[cb->fi - 1];
    memset(fr, 0, sizeof(*fr));
    fr->dport = ntohs(x->g->dport);
    fr->sport = ntohs(x->g->sport);
    fr->length = x->length;
    g_stat[4]++;
    if (!x->length) return; /* (nrecv's EOF) */
    const int whole = x->ncopy == x->length;
    if (whole && inpl) {
        fr->data = seg_payload(m, x->g);
        fr->mb = m[x->g->frame];
        mb_get(fr->mb);
    } else if (whole && pl_ref >= 0) {
        fr->data = (unsigned char *)payload + x->offset;
        cb->rb->pl_ref = pl_ref;
    } else {
        fr->data = cb->pp;
        if (payload) {
            memcpy(cb->pp, payload + x->offset, x->ncopy);
        } else {
            uint32_t pos = 0; /* of record j's bytes among the records' */
            for (uint32_t j = 0; j < x->nseg; j++) {
                const rxg_segment *g = &x->g[j];
                const uint32_t t = g->ncopy, lo = pos > x->skip ? pos : x->skip;
                if (pos + t > lo)
                    memcpy(cb->pp + (lo - x->skip),
                           seg_payload(m, g) + (x->tail ? (uint32_t)g->plen - t : 0u) + (lo - pos),
                           pos + t - lo);
                pos += t;
            }
        }
        if (x->length > x->ncopy) memset(cb->pp + x->ncopy, 0, x->length - x->ncopy);
        cb->pp += x->length;
        g_copied_bytes += x->length;
    }
}

/* the ACK behind it (ng_tcp_send_ackpkt, tcp.c:187-216), after rcv_nxt and
 * snd_nxt have moved; ports from g */
CONN_STEP void put_ack(struct conn_batch *cb, const struct tcp_stream *s, const rxg_segment *g) {
    if (cb->ai++ >= cb->atake || !cb->ab) return;
    struct tcp_fragment *a = &cb->ab->frag[cb->ai - 1];
    memset(a, 0, sizeof(*a));
    a->sport = g->dport;
    a->dport = g->sport;
    a->seqnum = s->snd_nxt;
    a->acknum = s->rcv_nxt;
    a->tcp_flags = TCP_ACK;
    a->windows = D_TCP_INITIAL_WINDOW;
    a->hdrlen_off = 0x50;
}

/* The segment form: every PSH segment makes a fragment (payload captured
 * whole: in place or in the held buffer, else copied) and an ACK, a FIN the
 * EOF fragment and an ACK.  Returns 0, or 1 for the frame-by-frame path.
 * Receive coalescing (run non-NULL: the connection's nr runs, run[].first
 * counted from sg - base): a run of more than one segment — in-sequence
 * PSH|ACK segments with equal ack, payloads captured whole and byte-contiguous
 * at the run's offset — makes one fragment of the run's bytes and one ACK,
 * whose acknum is rcv_nxt after the run: the ACK that closes the run in the
 * segment-by-segment order.  A run of one takes the segment's path.  A full
 * receive ring drops whole runs.  Connections on the frame-by-frame path are
 * never coalesced. */
static int deliver_tcp_conn(struct tcp_stream *s, const rxg_segment *sg, uint32_t k,
                            const rxg_tcp_run *run, uint32_t nr, uint32_t base,
                            const uint8_t *payload, int32_t pl_ref, rxg_mbuf *const *m,
                            uint8_t *handled, int *rc_out) {
    if (conn_claim(s, sg, k, handled, rc_out)) return 1;
    /* the fragments and ACKs the segments make, in order (the state changes
     * at most once: ESTABLISHED -> CLOSE_WAIT on a FIN) */
    uint32_t nfr = 0, nack = 0;
    uint64_t pbytes = 0;
    int st = s->status;
    const int inpl = g_inplace; /* payloads captured whole stay in their frames */
    uint32_t ri = 0; /* the run that holds segment j */
    for (uint32_t j = 0; j < k && st == TCP_STATUS_ESTABLISHED; j++) {
        if (run) {
            while (ri + 1 < nr && run[ri + 1].first - base <= j) ri++;
            if (run[ri].nseg > 1) { /* one fragment, one ACK for the run (j is its first) */
                nfr++, nack++;
                if (pl_ref < 0) pbytes += run[ri].bytes; /* (copied) */
                g_gro_absorbed += run[ri].nseg - 1;
                j += run[ri].nseg - 1;
                continue;
            }
        }
        if (sg[j].flags & TCP_PSH) {
            nfr++, nack++;
            if (sg[j].plen > 0 && (sg[j].ncopy != (uint32_t)sg[j].plen /* cut short */ ||
                                   (!inpl && pl_ref < 0)))
                pbytes += (uint64_t)sg[j].plen; /* (copied) */
        }
        if (sg[j].flags & TCP_FIN) nfr++, nack++, st = TCP_STATUS_CLOSE_WAIT;
    }
    if (!nfr) return 0;
    struct conn_batch cb;
    conn_open(&cb, s, nfr, nack, pbytes);
    ri = 0;
    for (uint32_t j = 0; j < k && s->status == TCP_STATUS_ESTABLISHED; j++) {
        const rxg_segment *g = &sg[j];
        if (run) {
            while (ri + 1 < nr && run[ri + 1].first - base <= j) ri++;
            if (run[ri].nseg > 1) { /* (j is the run's first segment) */
                const rxg_tcp_run *r = &run[ri];
                const struct frag_src x = {g, r->nseg, r->offset, r->bytes, r->bytes, 0, 0};
                put_frag(&cb, &x, payload, pl_ref, m, 0);
                s->rcv_nxt += r->bytes;
                s->snd_nxt = g->ack;
                put_ack(&cb, s, g);
                j += r->nseg - 1;
                continue;
            }
        }
        if (g->flags & TCP_PSH) { /* tcp.c:226-262 */
            const uint32_t len = g->plen > 0 ? (uint32_t)g->plen : 0u;
            const struct frag_src x = {g, 1, g->offset, len, g->ncopy, 0, 0};
            put_frag(&cb, &x, payload, pl_ref, m, inpl);
            s->rcv_nxt += (uint32_t)g->plen;
            s->snd_nxt = g->ack;
            put_ack(&cb, s, g);
        }
        if (g->flags & TCP_FIN) { /* tcp.c:264-294: CLOSE_WAIT, EOF, ACK */
            const struct frag_src eof = {g, 1, 0, 0, 0, 0, 0};
            s->status = TCP_STATUS_CLOSE_WAIT;
            put_frag(&cb, &eof, payload, pl_ref, m, 0);
            s->rcv_nxt += 1;
            s->snd_nxt = g->ack;
            put_ack(&cb, s, g);
        }
    }
    conn_close(&cb, s);
    if (st == TCP_STATUS_CLOSE_WAIT) restate_tcb(s, 0);
    return 0;
}

/* The stream form (stream assembly on): the connection's k ordered records
 * carry ncopy = take, and st[0..nst) are its streams (st[].first counted from
 * sg - base), each one a contiguous byte range at st[].offset of the payload
 * buffer.  The host rule of rxgpu.h ("TCP stream assembly") aligns every
 * stream with rcv_nxt: one receive fragment of the fresh bytes (in the held
 * buffer when there is one, else copied; host verdicts: gathered from the
 * frames, each record's skip passed over), the EOF fragment behind a FIN in
 * sequence, and one ACK per stream; a stream behind a hole only draws an ACK. */
static int deliver_tcp_conn_streams(struct tcp_stream *s, const rxg_segment *sg, uint32_t k,
                                    const rxg_tcp_stream *st, uint32_t nst, uint32_t base,
                                    const uint8_t *payload, int32_t pl_ref, rxg_mbuf *const *m,
                                    uint8_t *handled, int *rc_out) {
    if (conn_claim(s, sg, k, handled, rc_out)) return 1;
    if (s->status != TCP_STATUS_ESTABLISHED) return 0;
    /* the fragments and ACKs the streams make, in order */
    uint32_t nfr = 0, nack = 0, R = s->rcv_nxt;
    uint64_t pbytes = 0;
    for (uint32_t q = 0; q < nst; q++) {
        const int fin = (st[q].flags & RXG_STREAM_FIN) != 0;
        if (!st[q].bytes && !fin) continue; /* (pure ACKs) */
        nack++;
        const int32_t d = (int32_t)(R - st[q].seq);
        if (d < 0) continue;
        const uint32_t fresh = st[q].bytes > (uint32_t)d ? st[q].bytes - (uint32_t)d : 0;
        if (fresh) nfr++, R += fresh, pbytes += pl_ref < 0 ? fresh : 0;
        if (fin && (uint32_t)d <= st[q].bytes) {
            nfr++;
            break;
        }
    }
    if (!nack) return 0;
    struct conn_batch cb;
    conn_open(&cb, s, nfr, nack, pbytes);
    for (uint32_t q = 0; q < nst && s->status == TCP_STATUS_ESTABLISHED; q++) {
        const rxg_tcp_stream *x = &st[q];
        const rxg_segment *g = &sg[x->first - base], *gl = g + x->nseg - 1;
        const int fin = (x->flags & RXG_STREAM_FIN) != 0;
        /* payload a usable record carried and the device (or the host rule)
         * passed over: already held by an earlier segment of the burst */
        for (uint32_t j = 0; j < x->nseg; j++) {
            const uint32_t from = 34u + 4u * g[j].hl, cap = m[g[j].frame]->data_len;
            if (g[j].plen > 0 && !(g[j].flags & 0x06u) /* (not SYN, RST) */ && cap >= from &&
                cap - from >= (uint32_t)g[j].plen)
                g_asm_dup += (uint32_t)g[j].plen - g[j].ncopy;
        }
        if (!x->bytes && !fin) continue;
        const int32_t d = (int32_t)(s->rcv_nxt - x->seq);
        if (d >= 0) {
            const uint32_t fresh = x->bytes > (uint32_t)d ? x->bytes - (uint32_t)d : 0;
            g_asm_dup += x->bytes - fresh;
            if (fresh) {
                const uint32_t skip = (uint32_t)d;
                const struct frag_src f = {g, x->nseg, x->offset + skip, fresh, fresh, skip, 1};
                put_frag(&cb, &f, payload, pl_ref, m, 0);
                s->rcv_nxt += fresh;
            }
            if (fin && (uint32_t)d <= x->bytes) {
                const struct frag_src eof = {g, 1, 0, 0, 0, 0, 0};
                put_frag(&cb, &eof, payload, pl_ref, m, 0);
                s->status = TCP_STATUS_CLOSE_WAIT;
                s->rcv_nxt += 1;
            }
            s->snd_nxt = x->ack;
        } else {
            g_asm_hole++;
        }
        put_ack(&cb, s, gl);
    }
    conn_close(&cb, s);
    if (s->status == TCP_STATUS_CLOSE_WAIT) restate_tcb(s, 0);
    return 0;
}

/* the sorted segments, connection by connection (g_lock held); frames of
 * connections that need the frame-by-frame path are left unmarked */
static void deliver_tcp_sorted(const rxg_segment *sg, uint32_t nseg, const rxg_tcp_run *run,
                               uint32_t nrun, const struct asm_view *av, const uint8_t *payload,
                               int32_t pl_ref, rxg_mbuf *const *m, uint8_t *handled, int *rc_out) {
    uint32_t r0 = 0; /* (coalescing) the first run of the connection: runs never span two */
    uint32_t q0 = 0; /* (assembly) its first stream: streams never span two either */
    for (uint32_t a = 0, b; a < nseg; a = b) {
        b = a + 1;
        while (b < nseg && sg[b].flow == sg[a].flow) b++;
        /* look-ahead: the next connection's tcb and, in place, the mbufs of
         * the next segments (each gets a reference) */
        if (b < nseg && sg[b].flow < s_tcb_cap && s_tcb_cb[sg[b].flow])
            __builtin_prefetch(s_tcb_cb[sg[b].flow], 1, 0);
        if (g_inplace)
            for (uint32_t j = b; j < b + 8 && j < nseg; j++) __builtin_prefetch(m[sg[j].frame], 1, 0);
        struct tcp_stream *s = sg[a].flow < s_tcb_cap ? s_tcb_cb[sg[a].flow] : NULL;
        uint32_t r1 = r0;
        if (run)
            while (r1 < nrun && run[r1].first < b) r1++;
        uint32_t q1 = q0;
        if (av)
            while (q1 < av->n && av->st[q1].first < b) q1++;
        if (s && av)
            deliver_tcp_conn_streams(s, sg + a, b - a, av->st + q0, q1 - q0, a, payload, pl_ref, m,
                                     handled, rc_out);
        else if (s)
            deliver_tcp_conn(s, sg + a, b - a, run && r1 > r0 ? run + r0 : NULL, r1 - r0, a, payload,
                             pl_ref, m, handled, rc_out);
        r0 = r1;
        q0 = q1;
    }
}

/* ---- the host record pipeline (nstack_deliver) ----------------------------
 * The segment records of a burst whose verdicts came from elsewhere: the same
 * fields the GPU's segment sort decodes (rc-0 TCP verdicts naming a live tcb
 * id, bytes past the capture read as 0), stably sorted by tcb id on the host;
 * payloads are then copied from the frames */
static int seg_cmp(const void *a, const void *b) {
    const rxg_segment *x = a, *y = b;
    if (x->flow != y->flow) return x->flow < y->flow ? -1 : 1;
    return x->frame < y->frame ? -1 : (x->frame > y->frame);
}
static uint32_t host_segments(rxg_mbuf *const *m, uint32_t n, const rxg_verdict *v,
                              rxg_segment *sg) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (v[i].cls != RXG_CLS_TCP || v[i].rc != RXG_RC_OK || v[i].flow_id >= s_tcb_cap) continue;
        const uint8_t *f = (const uint8_t *)m[i]->buf_addr + m[i]->data_off;
        const uint32_t cap = m[i]->data_len;
#define B8(j) ((uint32_t)((j) < cap ? f[(j)] : 0u))
        rxg_segment *g = &sg[k++];
        memset(g, 0, sizeof(*g));
        g->frame = i;
        g->flow = v[i].flow_id;
        g->seq = B8(38) << 24 | B8(39) << 16 | B8(40) << 8 | B8(41);
        g->ack = B8(42) << 24 | B8(43) << 16 | B8(44) << 8 | B8(45);
        g->hl = (uint8_t)(B8(46) >> 4);
        g->flags = (uint8_t)B8(47);
        g->plen = (int32_t)(B8(16) << 8 | B8(17)) - 20 - 4 * (int32_t)g->hl;
        g->sport = (uint16_t)(B8(34) | B8(35) << 8);
        g->dport = (uint16_t)(B8(36) | B8(37) << 8);
#undef B8
        const uint32_t from = 34u + 4u * g->hl, avail = cap > from ? cap - from : 0u;
        if ((g->flags & TCP_PSH) && g->plen > 0)
            g->ncopy = (uint16_t)((uint32_t)g->plen < avail ? (uint32_t)g->plen : avail);
    }
    qsort(sg, k, sizeof(*sg), seg_cmp);
    return k;
}

/* What the device paths get from the library for deliver_tcp_sorted, built
 * on the host by the rules' host restatements: the sorted records; with
 * ordering or assembly on, in sequence order (assembly implies ordering);
 * with coalescing on, the runs; with assembly on, the streams, the records
 * then carrying ncopy = take as the device's do. */
struct host_records {
    rxg_segment *sg;
    uint32_t nseg;
    rxg_tcp_run *run; /* NULL: the segments one by one */
    uint32_t nrun;
    rxg_tcp_stream *stm;
    struct asm_view av; /* av.st NULL: assembly off */
};
static void host_records_free(struct host_records *hr) {
    free(hr->sg), free(hr->run), free(hr->stm);
    memset(hr, 0, sizeof(*hr));
}
/* Returns 0, or -1 (nothing left allocated) when memory ran out or a rule
 * refused the records: every TCP frame of the burst then takes the
 * frame-by-frame path, which validates it on its own. */
static int host_records_build(struct host_records *hr, rxg_mbuf *const *m, uint32_t n,
                              const rxg_verdict *v) {
    memset(hr, 0, sizeof(*hr));
    if (!(hr->sg = malloc((size_t)n * sizeof(*hr->sg)))) return -1;
    rxg_segment *sg = hr->sg;
    const uint32_t k = hr->nseg = host_segments(m, n, v, sg);
    if (!k || !(g_gro || g_order || g_assemble)) return 0;
    /* the rules' side arrays: the source addresses (read from the mbufs),
     * then 4k words of scratch (ordering: perm, sipo; assembly: avail and the
     * rule's three outputs) and the ordered copy of the records */
    uint32_t *sip = malloc((size_t)k * 5 * sizeof(*sip)), *w = sip ? sip + k : NULL;
    rxg_segment *so = g_order || g_assemble ? malloc((size_t)k * sizeof(*so)) : NULL;
    if (g_gro) hr->run = malloc((size_t)k * sizeof(*hr->run));
    if (g_assemble) hr->stm = malloc((size_t)k * sizeof(*hr->stm));
    int ok = sip && (so || !(g_order || g_assemble)) && (hr->run || !g_gro) &&
             (hr->stm || !g_assemble);
    if (ok) {
        for (uint32_t j = 0; j < k; j++) {
            const rxg_mbuf *mb = m[sg[j].frame];
            const uint8_t *f = (const uint8_t *)mb->buf_addr + mb->data_off;
            sip[j] = 0;
            for (uint32_t q = 0; q < 4; q++)
                if (26u + q < mb->data_len) sip[j] |= (uint32_t)f[26u + q] << (8u * q);
        }
        uint32_t moved = 0, *perm = w, *sipo = w + k;
        if (so && rxg_tcp_order_host(sg, sip, k, perm, &moved) == RXG_OK && moved) {
            for (uint32_t j = 0; j < k; j++) so[j] = sg[perm[j]], sipo[j] = sip[perm[j]];
            memcpy(sg, so, (size_t)k * sizeof(*sg));
            memcpy(sip, sipo, (size_t)k * sizeof(*sip));
            g_order_moved += moved;
        }
        if (hr->run && rxg_tcp_runs_host(sg, sip, k, g_gro, hr->run, &hr->nrun) != RXG_OK)
            hr->nrun = 0;
        if (hr->stm) {
            for (uint32_t j = 0; j < k; j++) {
                const uint32_t cap = m[sg[j].frame]->data_len, from = 34u + 4u * sg[j].hl;
                w[j] = cap > from ? cap - from : 0u;
            }
            uint32_t nst = 0;
            ok = rxg_tcp_assemble_host(sg, sip, w, k, hr->stm, &nst, w + k, w + 2 * k, w + 3 * k) ==
                 RXG_OK;
            for (uint32_t j = 0; ok && j < k; j++) sg[j].ncopy = (uint16_t)w[2 * k + j];
            hr->av.st = hr->stm, hr->av.n = nst;
        }
    }
    free(sip), free(so);
    if (!ok) host_records_free(hr);
    return ok ? 0 : -1;
}

/* ---- the burst-scoped state (g_lock held) ---------------------------------
 * burst_begin: the verdicts were made against the lists of generation gen
 * (another one: stale, every frame is looked up again); SYN cookies as the
 * alarm stood before this burst, no statuses yet.  burst_end: all of it, and
 * the mark that UDP went out as batches, cleared for the next burst. */
static void burst_begin(uint64_t gen) {
    g_burst_mutated = 0;
    g_burst_stale = gen != g_snap_gen;
    g_ck_on = ck_active();
    g_ck_st = NULL;
    if (g_ck_on) g_ck_p.t = ck_now();
}
static void burst_end(void) {
    g_udp_done = 0;
    g_burst_stale = 0;
    g_ck_on = 0, g_ck_st = NULL;
}

int nstack_deliver(rxg_mbuf *const *m, uint32_t n, const rxg_verdict *v, uint64_t gen,
                   int *rc_out) {
    if (!m || !v) return n ? RXG_EINVAL : 0;
    reclaim();
    pthread_mutex_lock(&g_lock);
    /* (refused while pipelined bursts are pending: their frames come first) */
    int rc = g_ctx && !g_pend_n ? RXG_OK : RXG_EINVAL;
    int delivered = 0;
    if (rc == RXG_OK) {
        burst_begin(gen);
        /* fresh: the verdicts' flow ids name the live blocks */
        const int fresh = !g_burst_stale && n;
        if (g_ck_on && fresh) ck_host_burst(m, n, v);
        if (g_ddos && n) ddos_host_burst(m, n); /* (sees the frames; changes nothing below) */
        if (g_l2 && n) l2_host_frames(m, n, v);  /* (the rule reads cls alone: stale or not) */
        rxg_dgram *dg = NULL;
        uint32_t *first = NULL;
        uint8_t *pl = NULL;
        if (fresh && host_dgrams(m, n, v, s_udp_cap, &dg, &first, &pl)) {
            delivered += deliver_udp_batches(m, dg, first, pl, s_udp_cap);
            g_udp_done = 1; /* the per-frame loop leaves UDP alone */
        }
        free(dg), free(first), free(pl);
        const uint8_t *done = NULL;
        struct host_records hr;
        if (fresh && !grow((void **)&s_handled, &s_handled_cap, n, 1) &&
            !host_records_build(&hr, m, n, v)) {
            memset(s_handled, 0, n);
            deliver_tcp_sorted(hr.sg, hr.nseg, hr.nrun ? hr.run : NULL, hr.nrun,
                               hr.av.st ? &hr.av : NULL, NULL, -1, m, s_handled, rc_out);
            host_records_free(&hr);
            done = s_handled;
        }
        delivered += deliver_burst(m, n, v, rc_out, done);
        burst_end();
        atomic_fetch_add_explicit(&g_deliveries, 1, memory_order_release);
    }
    pthread_mutex_unlock(&g_lock);
    return rc == RXG_OK ? delivered : rc;
}

/* the last nstack_rx_burst's phases (nstack_last_burst_phases) */
static float g_phase_ms[12];

static double mono_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

/* a delivered burst's phases: the device's five (HIP events; two halves
 * summed), the library calls (host clock), deliver_part's three, the call
 * since t0, the burst's segment and datagram records */
static void phases_record(const float *gms, const float *gms2, double lib_ms, const double ph[3],
                          double t0, const rxg_delivery *d, const rxg_delivery *d2) {
    for (int j = 0; j < 5; j++) g_phase_ms[j] = gms[j] + (gms2 ? gms2[j] : 0.0f);
    g_phase_ms[5] = (float)lib_ms;
    g_phase_ms[6] = (float)ph[0]; /* UDP batches to the sockets */
    g_phase_ms[7] = (float)ph[1]; /* TCP connections from the segment sort */
    g_phase_ms[8] = (float)ph[2]; /* the frame-by-frame loop (the rest) */
    g_phase_ms[9] = (float)(mono_ms() - t0);
    g_phase_ms[10] = (float)(d->nseg + (d2 ? d2->nseg : 0));
    g_phase_ms[11] = (float)(d->ndgram + (d2 ? d2->ndgram : 0));
}

/* a pooled payload buffer the library can take for the next submit (set
 * g_next_set releases its own previous one): none held by queued batches and
 * none the other sets' last bursts used */
static int pl_free(void) {
    for (int k = 0; k < RXG_PAYLOAD_BUFS; k++) {
        if (atomic_load_explicit(&g_pl_out[k], memory_order_acquire)) continue;
        int held = 0;
        for (uint32_t j = 0; j < RXG_DELIVER_DEPTH; j++)
            if (j != g_next_set && g_set_ref[j] == k) held = 1;
        if (!held) return 1;
    }
    return 0;
}

/* g_lock held by the protocol thread: while an application thread drains and
 * every pooled buffer is still held by its unread batches, wait for one (the
 * lock released, so the application can take fragments out), up to 20 ms;
 * past that the library's set buffer is used and the payloads copied */
static void pl_wait_free(void) {
    if (!atomic_load_explicit(&g_drainers, memory_order_relaxed) || pl_free()) return;
    const double t0 = mono_ms();
    g_pl_waits++;
    atomic_store_explicit(&g_pl_waiting, 1, memory_order_seq_cst);
    while (!pl_free() && atomic_load_explicit(&g_drainers, memory_order_relaxed) &&
           mono_ms() - t0 < 20.0) {
        pthread_mutex_unlock(&g_lock);
        reclaim(); /* (the batches the application let go of free their buffers here) */
        pthread_mutex_lock(&g_pl_mx);
        if (!pl_free() && !atomic_load_explicit(&g_frag_garbage, memory_order_seq_cst)) {
            struct timespec ts;
            clock_gettime(CLOCK_REALTIME, &ts);
            ts.tv_nsec += 1000000;
            if (ts.tv_nsec >= 1000000000) ts.tv_sec++, ts.tv_nsec -= 1000000000;
            pthread_cond_timedwait(&g_pl_cv, &g_pl_mx, &ts);
        }
        pthread_mutex_unlock(&g_pl_mx);
        proto_lock();
    }
    atomic_store_explicit(&g_pl_waiting, 0, memory_order_relaxed);
}

/* after a submit: the set it took and the pooled buffer (or -1) it holds */
static void pl_note_submit(const rxg_delivery *d) {
    if (d->set < 1 || d->set > RXG_DELIVER_DEPTH) return;
    g_set_ref[d->set - 1] = d->tcp_payload_ref;
    g_next_set = d->set % RXG_DELIVER_DEPTH;
}

int nstack_set_halves(uint32_t min_half) {
    pthread_mutex_lock(&g_lock);
    g_half_min = min_half;
    pthread_mutex_unlock(&g_lock);
    return RXG_OK;
}

/* g_lock held: deliver one part of a burst the GPU has classified (`d`, its
 * verdicts `v`), submitted when the lookups' snapshot generation was gen0 —
 * the UDP batches, the sorted TCP connections, then the frame-by-frame rest;
 * ph[3] += the three phases' times.  Returns the UDP datagrams delivered. */
static int deliver_part(rxg_mbuf *const *m, uint32_t k, const rxg_verdict *v, uint8_t *handled,
                        int *rco, rxg_delivery *d, uint64_t gen0, double ph[3]) {
    int delivered = 0;
    const double t1 = mono_ms();
    burst_begin(gen0);
    if (g_burst_stale) { /* (ids may name other blocks now) */
        d->first = NULL, d->nseg = 0;
        g_stale_parts++;
    }
    if (d->first) {
        delivered += deliver_udp_batches(m, d->dgram, d->first, d->udp_payload, rxg_num_udp_ids(g_ctx));
        g_udp_done = 1; /* the per-frame loop leaves UDP alone */
    }
    const double t2 = mono_ms();
    memset(handled, 0, k);
    const rxg_tcp_run *run = NULL; /* (coalescing on at the submit: the burst's runs) */
    uint32_t nrun = 0;
    if (d->nseg && g_gro && rxg_delivery_runs(g_ctx, d, &run, &nrun) != RXG_OK) run = NULL, nrun = 0;
    uint32_t moved = 0; /* (ordering on at the submit: the records that moved) */
    if (d->nseg && (g_order || g_assemble) && rxg_delivery_moved(g_ctx, d, &moved) == RXG_OK) g_order_moved += moved;
    /* SYN cookies on: the burst's statuses, descriptors and totals when K7 ran
     * at the submit and the verdicts' ids still name the live blocks */
    if (g_ck_on) {
        const rxg_txd *ctxd = NULL;
        uint32_t cn = 0, ctot[4];
        if (!g_burst_stale && rxg_delivery_cookies(g_ctx, d, &g_ck_st, &ctxd, &cn, ctot) == RXG_OK &&
            g_ck_st)
            ck_take(ctxd, ctot);
        else
            g_ck_st = NULL;
    }
    /* the L2 responder: the burst's answers when K8 ran at the submit, else the
     * frames one by one */
    if (g_l2) {
        const uint8_t *lst = NULL, *lfr = NULL;
        const uint32_t *lro = NULL, *lrs = NULL;
        const uint16_t *lrl = NULL;
        uint32_t lna = 0, ltot[6];
        if (!g_burst_stale && rxg_delivery_l2(g_ctx, d, &lst, &lfr, &lro, &lrl, &lrs, &lna, ltot) == RXG_OK &&
            lst)
            l2_take(lst, lfr, lro, lrl, lrs, lna, ltot);
        else
            l2_host_frames(m, k, v);
    }
    rxg_ddos_summary dsum; /* (the detector on at the submit: the burst's summary) */
    if (g_ddos && rxg_delivery_ddos(g_ctx, d, &dsum) == RXG_OK) ddos_account(&dsum);
    struct asm_view av = {NULL, 0}; /* (assembly on at the submit: the burst's streams) */
    if (d->nseg && g_assemble && rxg_delivery_streams(g_ctx, d, &av.st, &av.n) != RXG_OK) av.st = NULL;
    if (d->nseg && (!g_assemble || av.st))
        deliver_tcp_sorted(d->seg, d->nseg, nrun ? run : NULL, nrun, av.st ? &av : NULL,
                           d->tcp_payload, d->tcp_payload_ref, m, handled, rco);
    const double t3 = mono_ms();
    delivered += deliver_burst(m, k, v, rco, handled);
    burst_end();
    const double t4 = mono_ms();
    ph[0] += t2 - t1, ph[1] += t3 - t2, ph[2] += t4 - t3;
    return delivered;
}

int nstack_rx_burst(rxg_mbuf *const *m, uint32_t n, int *rc_out, rxg_verdict *v_out) {
    if (!m && n) return RXG_EINVAL;
    t_proto = 1;
    /* the garbage lists are freed below, while the burst is on the GPU; with
     * pooled payload buffers (not in place) first, since the submit picks a
     * buffer and the batches the application let go of may be what holds one */
    if (!g_inplace) reclaim();
    proto_lock();
    pl_wait_free(); /* (two threads: the application frees the payload buffers) */
    const double t0 = mono_ms();
    /* one protocol thread (the reference's pkt_process lcore): a second
     * rx_burst while one waits for the GPU is refused */
    int rc = g_ctx && !g_rx_in_flight && !g_pend_n ? RXG_OK : RXG_EINVAL;
    if (rc == RXG_OK && grow((void **)&s_v, &s_v_cap, n ? n : 1, sizeof(rxg_verdict)))
        rc = RXG_ENOMEM;
    if (rc == RXG_OK && grow((void **)&s_handled, &s_handled_cap, n ? n : 1, 1)) rc = RXG_ENOMEM;
    /* the device half of delivery: classify, UDP payloads grouped per socket
     * (<= RXG_COMPACT_MAX_FLOWS ids: always, with the reference's 1024
     * descriptors), TCP segments sorted per connection with their payloads
     * gathered.  While it runs on the GPU the stack's lock is free: the
     * application's socket calls proceed (the reference's app lcore runs
     * beside its protocol lcore).  If the blocks changed meanwhile — by those
     * calls, or by the first half's own segments (a SYN, a last ACK) — a half
     * is delivered like verdicts of an older snapshot: frame by frame, every
     * lookup made again on the live lists, which is the reference's sequential
     * outcome. */
    const uint32_t nh = g_half_min && n >= 2 * g_half_min ? n / 2 : n;
    const uint32_t part_off[2] = {0, nh}, part_n[2] = {nh, n - nh};
    const int parts = nh < n ? 2 : 1;
    rxg_delivery d[2];
    float gms[2][8];
    memset(gms, 0, sizeof(gms));
    int sub[2] = {0, 0};
    const uint64_t gen0 = g_snap_gen;
    double lib_ms = 0;
    if (rc == RXG_OK && g_ck_mode) (void)rxg_syncookie_tick(g_ctx, ck_now());
    /* both halves go out before the first is waited for; a second half the
     * library refused is submitted again once the first is delivered */
    for (int h = 0; rc == RXG_OK && h < parts; h++) {
        const double a = mono_ms();
        const int src = rxg_deliver_submit(g_ctx, m + part_off[h], part_n[h], s_v + part_off[h], &d[h]);
        lib_ms += mono_ms() - a;
        pl_note_submit(&d[h]);
        if (src == RXG_OK)
            sub[h] = 1;
        else if (h == 0)
            rc = src;
    }
    rxg_ctx *ctx = g_ctx;
    int delivered = 0;
    int done[2] = {0, 0}; /* half delivered */
    double ph[3] = {0, 0, 0};
    if (sub[0]) g_rx_in_flight = 1;
    for (int h = 0; h < parts && (sub[h] || rc == RXG_OK); h++) {
        const uint32_t o = part_off[h], k = part_n[h];
        if (!sub[h]) { /* (the lock is held here) */
            const double a = mono_ms();
            rc = rxg_deliver_submit(g_ctx, m + o, k, s_v + o, &d[h]);
            lib_ms += mono_ms() - a;
            pl_note_submit(&d[h]);
            if (rc != RXG_OK) break;
            sub[h] = 1;
        }
        pthread_mutex_unlock(&g_lock);
        /* what the application threads let go of (batches, frame references)
         * is freed here, while the first half is on the GPU: with the
         * application on its own core those frees pull cache lines from it
         * (0.5-0.6 ms per 16K-segment burst, profiles/r05d), time the wait
         * below would otherwise spend idle */
        if (h == 0) reclaim();
        const double a = mono_ms();
        const int wrc = rxg_deliver_wait(ctx, &d[h], gms[h]);
        lib_ms += mono_ms() - a;
        proto_lock();
        if (rc == RXG_OK) rc = wrc;
        if (rc != RXG_OK) continue; /* (a submitted half is still waited for) */
        delivered += deliver_part(m + o, k, s_v + o, s_handled + o, rc_out ? rc_out + o : NULL,
                                  &d[h], gen0, ph);
        done[h] = 1;
    }
    g_rx_in_flight = 0;
    /* the first half delivered, the second not put through the GPU (a failed
     * second submit or wait): its frames are reported, not delivered.  Only a
     * caller that passed rc_out can see that per frame; without it the call
     * returns the error code, as a whole-burst failure does */
    const int partial = rc != RXG_OK && parts > 1 && done[0] && !done[1] && rc_out;
    if (partial) {
        for (uint32_t i = nh; i < n; i++) rc_out[i] = rc;
        if (v_out) memset(v_out + nh, 0, (size_t)(n - nh) * sizeof(rxg_verdict));
    }
    if (rc == RXG_OK || partial) {
        if (v_out) memcpy(v_out, s_v, (size_t)(partial ? nh : n) * sizeof(rxg_verdict));
        phases_record(gms[0], gms[1], lib_ms, ph, t0, &d[0], parts > 1 ? &d[1] : NULL);
    }
    if (done[0]) atomic_fetch_add_explicit(&g_deliveries, 1, memory_order_release);
    pthread_mutex_unlock(&g_lock);
    return rc == RXG_OK || partial ? delivered : rc;
}

/* ---- pipelined receive: one burst on the GPU while the last is delivered --
 * The reference's protocol lcore takes a burst and runs every frame through
 * udp_process / tcp_process before it takes the next (netfamily.c:147-200).
 * nstack_rx_submit / nstack_rx_complete keep that order of delivery but let
 * burst k+1 cross PCIe and go through K1/K3/K4 while burst k is delivered
 * (the library's delivery sets, RXG_DELIVER_DEPTH).  A burst submitted before
 * the previous one was delivered was classified against the lookups of its
 * submit: when that delivery (a SYN, a last ACK) or a socket call moved a
 * lookup, the burst is delivered frame by frame on the live lists
 * (deliver_part's stale path), the reference's sequential outcome. */

/* the protocol thread: wait for a pending burst's device half (no lock:
 * only this thread touches the pending bursts) */
static void pend_wait(struct rx_pend *p) {
    if (p->waited) return;
    const double a = mono_ms();
    p->wrc = rxg_deliver_wait(g_ctx, &p->d, p->gms);
    p->lib_ms += mono_ms() - a;
    p->waited = 1;
}

int nstack_rx_submit(rxg_mbuf *const *m, uint32_t n, int *rc_out, rxg_verdict *v_out) {
    if (!m && n) return RXG_EINVAL;
    t_proto = 1;
    /* the bursts already on the GPU are waited for first: their results'
     * copies back were queued behind their kernels, and this burst's copy in
     * (0.57 ms at cfg3) would otherwise go ahead of them, so their
     * completes waited for it (r06d: lib_call 0.66 ms per pipelined burst).
     * A burst submitted one delivery earlier is normally done by now. */
    if (g_ctx)
        for (uint32_t j = 0; j < g_pend_n; j++) pend_wait(&g_pend[(g_pend_head + j) % RXG_DELIVER_DEPTH]);
    if (!g_inplace) reclaim();
    proto_lock();
    pl_wait_free();
    int rc = g_ctx && !g_rx_in_flight && g_pend_n < RXG_DELIVER_DEPTH ? RXG_OK : RXG_EINVAL;
    struct rx_pend *p = &g_pend[(g_pend_head + g_pend_n) % RXG_DELIVER_DEPTH];
    if (rc == RXG_OK && (grow((void **)&p->v, &p->v_cap, n ? n : 1, sizeof(rxg_verdict)) ||
                         grow((void **)&p->handled, &p->h_cap, n ? n : 1, 1)))
        rc = RXG_ENOMEM;
    if (rc == RXG_OK) {
        p->m = m, p->n = n, p->rc_out = rc_out, p->v_out = v_out;
        p->gen0 = g_snap_gen;
        p->waited = 0;
        if (g_ck_mode) (void)rxg_syncookie_tick(g_ctx, ck_now());
        memset(p->gms, 0, sizeof(p->gms));
        const double a = mono_ms();
        rc = rxg_deliver_submit(g_ctx, m, n, p->v, &p->d);
        p->lib_ms = mono_ms() - a;
        pl_note_submit(&p->d);
        if (rc == RXG_OK) g_pend_n++;
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_rx_pending(void) {
    proto_lock();
    const int k = (int)g_pend_n;
    pthread_mutex_unlock(&g_lock);
    return k;
}

int nstack_rx_complete(void) {
    t_proto = 1;
    const double t0 = mono_ms();
    proto_lock();
    if (!g_pend_n || !g_ctx) {
        pthread_mutex_unlock(&g_lock);
        return RXG_EINVAL;
    }
    struct rx_pend *p = &g_pend[g_pend_head];
    pthread_mutex_unlock(&g_lock);
    /* what the application threads let go of is freed while the burst (and
     * the one submitted after it) is on the GPU */
    reclaim();
    pend_wait(p);
    const int wrc = p->wrc;
    const float *gms = p->gms;
    const double lib_ms = p->lib_ms;
    proto_lock();
    g_pend_head = (g_pend_head + 1) % RXG_DELIVER_DEPTH;
    g_pend_n--;
    if (wrc != RXG_OK) { /* the burst is not delivered: the caller may pass its frames again */
        pthread_mutex_unlock(&g_lock);
        return wrc;
    }
    double ph[3] = {0, 0, 0};
    const int delivered = deliver_part(p->m, p->n, p->v, p->handled, p->rc_out, &p->d, p->gen0, ph);
    if (p->v_out) memcpy(p->v_out, p->v, (size_t)p->n * sizeof(rxg_verdict));
    phases_record(gms, NULL, lib_ms, ph, t0 /* (the submit is the caller's) */, &p->d, NULL);
    atomic_fetch_add_explicit(&g_deliveries, 1, memory_order_release);
    pthread_mutex_unlock(&g_lock);
    return delivered;
}

int nstack_last_burst_phases(float ms[12]) {
    if (!ms) return RXG_EINVAL;
    /* read by the protocol thread between its bursts: it goes ahead of an
     * application loop (drain_all) as rx_burst itself does */
    proto_lock();
    memcpy(ms, g_phase_ms, sizeof(g_phase_ms));
    pthread_mutex_unlock(&g_lock);
    return RXG_OK;
}

int nstack_tcb_state(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport, int32_t *status,
                     uint32_t *rcv_nxt, uint32_t *snd_nxt, int32_t *fd) {
    pthread_mutex_lock(&g_lock);
    int rc = -1;
    for (struct tcp_stream *s = g_tcb_set; s; s = s->next)
        if (s->sip == sip && s->dip == dip && s->sport == sport && s->dport == dport) {
            if (status) *status = (int32_t)s->status;
            if (rcv_nxt) *rcv_nxt = s->rcv_nxt;
            if (snd_nxt) *snd_nxt = s->snd_nxt;
            if (fd) *fd = s->fd;
            rc = 0;
            break;
        }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_tcb_sndq(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport, uint32_t k,
                    uint8_t *flags, uint32_t *acknum) {
    pthread_mutex_lock(&g_lock);
    int rc = -1;
    for (struct tcp_stream *s = g_tcb_set; s; s = s->next)
        if (s->sip == sip && s->dip == dip && s->sport == sport && s->dport == dport) {
            pthread_mutex_lock(&s->mutex);
            const struct tcp_fragment *f = tq_at(s->sndbuf, k);
            if (f) {
                if (flags) *flags = f->tcp_flags;
                if (acknum) *acknum = f->acknum;
                rc = 0;
            }
            pthread_mutex_unlock(&s->mutex);
            break;
        }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

uint32_t nstack_tcb_count(void) {
    pthread_mutex_lock(&g_lock);
    uint32_t n = 0;
    for (struct tcp_stream *s = g_tcb_set; s; s = s->next) n++;
    pthread_mutex_unlock(&g_lock);
    return n;
}

int nstack_tcb_add(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport, int status) {
    pthread_mutex_lock(&g_lock);
    struct tcp_stream *s = g_ctx ? tcb_new(sip, dip, sport, dport, status) : NULL;
    if (!s) {
        pthread_mutex_unlock(&g_lock);
        return -1;
    }
    if (reg_tcb(s)) {
        ring_free(s->rcvbuf);
        ring_free(s->sndbuf);
        free(s);
        pthread_mutex_unlock(&g_lock);
        return -1;
    }
    LL_ADD(s, g_tcb_set); /* tcp.c:52 */
    if (status == TCP_STATUS_LISTEN) (void)ck_sync_listeners();
    wake_acceptors(dport);
    pthread_mutex_unlock(&g_lock);
    return 0;
}

int nstack_flows(rxg_udp_sock *u, uint32_t cap_u, uint32_t *nu, rxg_tcb *t, uint32_t cap_t,
                 uint32_t *nt, uint64_t *gen) {
    pthread_mutex_lock(&g_lock);
    int rc = g_ctx ? RXG_OK : RXG_EINVAL;
    if (rc == RXG_OK && g_dirty) rc = snapshot();
    if (rc == RXG_OK) {
        if (nu) *nu = s_nu;
        if (nt) *nt = s_nt;
        if (gen) *gen = g_snap_gen;
        if (u) memcpy(u, s_udp, (size_t)(s_nu < cap_u ? s_nu : cap_u) * sizeof(*u));
        if (t) memcpy(t, s_tcb, (size_t)(s_nt < cap_t ? s_nt : cap_t) * sizeof(*t));
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

/* FNV-1a 64 of a fragment's bytes: nstack_drain_all_sum adds them up, an
 * order-free check of what the application read (tests) */
static uint64_t fnv64(const void *p, size_t n) {
    const unsigned char *c = p;
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ c[i]) * 0x100000001b3ull;
    return h;
}

/* what drain_all took out of the tcbs it visited, read after their mutexes
 * are released */
struct drain_scratch {
    void **det; /* ring items taken out */
    uint32_t nd, det_cap;
    const unsigned char **fp; /* their fragments, flattened */
    uint32_t *fl, fcap;
};

/* the detached items read: each fragment counted (EOF fragments are read and
 * not counted), copied into buf, hashed (hs non-NULL), then the items freed
 * (a batch's hold on a payload buffer or on its frames' mbufs ends there).
 * The fragments lie scattered (in place: in their frames), so the copy loop
 * prefetches the lines of the fragment DRAIN_AHEAD places ahead. */
#ifndef NSTACK_DRAIN_AHEAD /* (tools/Makefile builds variants for tools/sock_host_bench) */
#define NSTACK_DRAIN_AHEAD 4
#endif
#ifndef NSTACK_DRAIN_LOC
#define NSTACK_DRAIN_LOC 0
#endif
static void drain_detached(struct drain_scratch *sc, void *buf, uint64_t *got, uint64_t *nb,
                           uint64_t *hs) {
    enum { DRAIN_AHEAD = NSTACK_DRAIN_AHEAD };
    uint32_t m = 0;
    for (uint32_t i = 0; i < sc->nd; i++) {
        const struct tcp_fragment *f = sc->det[i];
        const uint32_t a = f->batch ? f->batch->next : 0, n = f->batch ? f->batch->n : 1;
        if (m + (n - a) > sc->fcap) {
            uint32_t c1 = sc->fcap, c2 = sc->fcap;
            if (grow((void **)&sc->fp, &c1, m + (n - a), sizeof(*sc->fp)) ||
                grow((void **)&sc->fl, &c2, m + (n - a), sizeof(*sc->fl))) {
                m = 0; /* (out of memory: read without the flat list) */
                break;
            }
            sc->fcap = c1 < c2 ? c1 : c2;
        }
        for (uint32_t j = a; j < n; j++) {
            const struct tcp_fragment *g = f->batch ? &f->batch->frag[j] : f;
            sc->fp[m] = g->data;
            sc->fl[m++] = g->length;
        }
    }
    for (uint32_t i = 0; i < m; i++) {
        if (i + DRAIN_AHEAD < m && sc->fl[i + DRAIN_AHEAD]) {
            const uintptr_t p0 = (uintptr_t)sc->fp[i + DRAIN_AHEAD] & ~(uintptr_t)63;
            const uintptr_t p1 = (uintptr_t)sc->fp[i + DRAIN_AHEAD] + sc->fl[i + DRAIN_AHEAD];
            for (uintptr_t q = p0; q < p1; q += 64) __builtin_prefetch((const void *)q, 0, NSTACK_DRAIN_LOC);
        }
        if (sc->fl[i]) {
            memcpy(buf, sc->fp[i], sc->fl[i]);
            (*got)++, *nb += sc->fl[i];
            if (hs) *hs += fnv64(buf, sc->fl[i]);
        }
    }
    for (uint32_t i = 0; i < sc->nd; i++) {
        struct tcp_fragment *f = sc->det[i];
        if (!m) { /* (the fallback: fragment by fragment) */
            const uint32_t a = f->batch ? f->batch->next : 0, n = f->batch ? f->batch->n : 1;
            for (uint32_t j = a; j < n; j++) {
                const struct tcp_fragment *g = f->batch ? &f->batch->frag[j] : f;
                if (g->length) {
                    memcpy(buf, g->data, g->length);
                    (*got)++, *nb += g->length;
                    if (hs) *hs += fnv64(buf, g->length);
                }
            }
        }
        frag_item_free(f);
    }
    sc->nd = 0;
}

/* one UDP socket's receive ring emptied (its reference held): its items are
 * taken out under one hold of its mutex and read after it is released, each
 * datagram as udp_recv returns it (common.c:558-564: the captured payload,
 * then zeros to dgram_len); with a buffer shorter than a datagram can be
 * (cap < 65535), an item holding one that does not fit, and everything after
 * it, is read through udp_recv's split path instead */
static void drain_udp(struct localhost *h, void *buf, size_t cap, uint64_t *got, uint64_t *nb,
                      uint64_t *hs, struct drain_scratch *sc) {
    struct offload *o;
    uint32_t taken = 0;
    pthread_mutex_lock(&h->mutex);
    while (!h->dead && ring_peek(h->rcvbuf, (void **)&o) == 0) {
        const uint32_t a = o->batch ? o->batch->next : 0, n = o->batch ? o->batch->n : 1;
        if (cap < 65535u) {
            uint32_t j = a;
            while (j < n && (o->batch ? (size_t)o->batch->meta[j].len + 8u : (size_t)o->length) <= cap) j++;
            if (j < n) break;
        }
        if (sc->nd == sc->det_cap &&
            grow((void **)&sc->det, &sc->det_cap, sc->det_cap ? 2 * sc->det_cap : 256, sizeof(void *)))
            break;
        ring_dequeue(h->rcvbuf, (void **)&o);
        sc->det[sc->nd++] = o;
        taken += n - a;
    }
    cnt_set(&h->queued, h->queued - taken);
    pthread_mutex_unlock(&h->mutex);
    unsigned char *out = buf;
    for (uint32_t i = 0; i < sc->nd; i++) {
        o = sc->det[i];
        if (o->batch) {
            const struct dgram_batch *b = o->batch;
            for (uint32_t j = b->next; j < b->n; j++) {
                const struct dgram_meta *d = &b->meta[j];
                const uint32_t length = (uint32_t)d->len + 8u; /* (udp.c:37) */
                memcpy(out, b->data + d->off, d->ncopy);
                memset(out + d->ncopy, 0, length - d->ncopy);
                (*got)++, *nb += length;
                if (hs) *hs += fnv64(out, length);
            }
        } else {
            memcpy(out, o->data, o->length);
            (*got)++, *nb += o->length;
            if (hs) *hs += fnv64(out, o->length);
        }
        offload_free(o);
    }
    sc->nd = 0;
    ssize_t r; /* (what did not fit, and what arrived meanwhile) */
    struct sockaddr_in sa;
    while ((r = udp_recv(h, buf, cap, MSG_DONTWAIT, (struct sockaddr *)&sa)) >= 0) {
        (*got)++, *nb += (uint64_t)r;
        if (hs) *hs += fnv64(buf, (size_t)r < cap ? (size_t)r : cap);
    }
}

/* one tcb's receive ring emptied (its reference held): its items are taken
 * out under one hold of its mutex, to be read after it is released
 * (drain_detached); an item with a fragment longer than `cap` is read in
 * place through nrecv's split path */
static void drain_tcb(struct tcp_stream *s, void *buf, size_t cap, uint64_t *got, uint64_t *nb,
                      uint64_t *hs, struct drain_scratch *sc) {
    struct tcp_fragment *f;
    pthread_mutex_lock(&s->mutex);
    while (!s->dead && ring_peek(s->rcvbuf, (void **)&f) == 0) {
        const uint32_t first = f->batch ? f->batch->next : 0, n = f->batch ? f->batch->n : 1;
        uint32_t j = first;
        while (j < n && (f->batch ? f->batch->frag[j].length : f->length) <= cap) j++;
        if (j < n || (sc->nd == sc->det_cap &&
                      grow((void **)&sc->det, &sc->det_cap, sc->det_cap ? 2 * sc->det_cap : 256,
                           sizeof(void *)))) {
            struct tcp_fragment *h = tq_front(s->rcvbuf);
            if (h->length > cap) {
                pthread_mutex_unlock(&s->mutex);
                const ssize_t r = nrecv_tcb(s, buf, cap, MSG_DONTWAIT);
                if (r > 0) {
                    (*got)++, *nb += (uint64_t)r;
                    if (hs) *hs += fnv64(buf, cap);
                }
                pthread_mutex_lock(&s->mutex);
                continue;
            }
            if (h->length) {
                memcpy(buf, h->data, h->length);
                (*got)++, *nb += h->length;
                if (hs) *hs += fnv64(buf, h->length);
            }
            tq_pop(s->rcvbuf, &s->rq);
            continue;
        }
        ring_dequeue(s->rcvbuf, (void **)&f);
        cnt_set(&s->rq, s->rq - (n - first));
        sc->det[sc->nd++] = f;
    }
    tq_clear(s->sndbuf, &s->sq); /* its queued control fragments (ACKs) sent */
    pthread_mutex_unlock(&s->mutex);
}

static int64_t drain_impl(void *buf, size_t cap, uint64_t *bytes, uint64_t *sum) {
    /* The application side of the benchmark: every socket read until empty,
     * EOF fragments read and not counted (as oracle_drain_all).  Blocks are
     * visited by stable id.  Only the id maps' lock (g_tab, never the
     * stack's lock) is held, to take a reference on the next DRAIN_CHUNK
     * live blocks (one hold for up to 8192 blocks) (a block stays valid
     * while referenced, even if the protocol thread frees it meanwhile: its
     * memory goes with the last reference); everything else — the rings, the
     * copies — runs under each block's own mutex, beside the protocol
     * thread's deliveries (the reference's app lcore reads its socket rings
     * beside the protocol lcore, netfamily.c:424-430, udp.c:48,
     * common.c:531-536). */
    enum { DRAIN_CHUNK = 8192 };
    void **blk = malloc(DRAIN_CHUNK * sizeof(void *));
    if (!blk) return RXG_ENOMEM;
    uint64_t got = 0, nb = 0, hs = 0;
    uint64_t *hp = sum ? &hs : NULL;
    struct drain_scratch sc;
    memset(&sc, 0, sizeof(sc));
    atomic_fetch_add_explicit(&g_drainers, 1, memory_order_relaxed);
    for (int kind = 0; kind < 2; kind++) {
        uint32_t id = 0;
        for (int more = 1; more;) {
            const double w0 = mono_ms();
            const double w1 = w0;
            pthread_mutex_lock(&g_tab); /* (not g_lock: see g_tab) */
            const double w2 = mono_ms();
            atomic_fetch_add_explicit(&g_drain_ns[1], (long long)((w1 - w0) * 1e6), memory_order_relaxed);
            atomic_fetch_add_explicit(&g_drain_ns[0], (long long)((w2 - w1) * 1e6), memory_order_relaxed);
            const uint32_t ncap = kind ? s_tcb_cap : s_udp_cap;
            uint32_t k = 0;
            for (; id < ncap && k < DRAIN_CHUNK; id++) {
                /* a block with nothing queued is passed over without a
                 * reference (its counters read, not its reference count
                 * written: the protocol thread keeps the line) */
                if (kind) {
                    struct tcp_stream *t = s_tcb_cb[id];
                    if (!t || (!cnt_peek(&t->rq) && !cnt_peek(&t->sq))) continue;
                    cb_get(&t->ref);
                    blk[k++] = t;
                } else {
                    struct localhost *h = s_udp_cb[id];
                    if (!h || !cnt_peek(&h->queued)) continue;
                    cb_get(&h->ref);
                    blk[k++] = h;
                }
            }
            more = id < ncap;
            pthread_mutex_unlock(&g_tab);
            const double c0 = mono_ms();
            for (uint32_t i = 0; i < k; i++) {
                /* look-ahead (every address formed from memory this call keeps
                 * alive: the referenced blocks, their rings and slot arrays,
                 * which live as long as the block; no ring item is read): the
                 * block 4 ahead, the ring of the one 2 ahead, and the head item
                 * of the next one's ring — its lines prefetched as they lie,
                 * a fragment batch's header and first fragments (frag_batch:
                 * the item, then its fragments), whatever the head slot holds
                 * by the time it is read */
                if (i + 4 < k)
                    for (int q = 0; q < 3; q++) __builtin_prefetch((const char *)blk[i + 4] + 64 * q, 0, 0);
                if (i + 2 < k)
                    __builtin_prefetch(kind ? (void *)((struct tcp_stream *)blk[i + 2])->rcvbuf
                                            : (void *)((struct localhost *)blk[i + 2])->rcvbuf,
                                       0, 0);
                if (kind && i + 1 < k) {
                    struct nring *r = ((struct tcp_stream *)blk[i + 1])->rcvbuf;
                    const uint32_t hd = __atomic_load_n(&r->head, __ATOMIC_RELAXED);
                    const char *it = (const char *)__atomic_load_n(&r->slot[hd % r->cap], __ATOMIC_RELAXED);
                    if (it)
                        for (int q = 0; q < 8; q++) __builtin_prefetch(it + 64 * q, 0, 0);
                }
                if (kind) {
                    drain_tcb(blk[i], buf, cap, &got, &nb, hp, &sc);
                    tcb_put(blk[i]); /* (the items taken out are this call's) */
                    if (sc.nd >= 256 || i + 1 == k) drain_detached(&sc, buf, &got, &nb, hp);
                } else {
                    drain_udp(blk[i], buf, cap, &got, &nb, hp, &sc);
                    udp_put(blk[i]);
                }
            }
            atomic_fetch_add_explicit(&g_drain_ns[2], (long long)((mono_ms() - c0) * 1e6), memory_order_relaxed);
        }
    }
    free(sc.det);
    free(sc.fp);
    free(sc.fl);
    free(blk);
    atomic_fetch_sub_explicit(&g_drainers, 1, memory_order_relaxed);
    pthread_mutex_lock(&g_pl_mx); /* a waiting protocol thread re-checks */
    pthread_cond_broadcast(&g_pl_cv);
    pthread_mutex_unlock(&g_pl_mx);
    if (bytes) *bytes = nb;
    if (sum) *sum = hs;
    return (int64_t)got;
}

int64_t nstack_drain_all(void *buf, size_t cap, uint64_t *bytes) {
    return drain_impl(buf, cap, bytes, NULL);
}

int64_t nstack_drain_all_sum(void *buf, size_t cap, uint64_t *bytes, uint64_t *sum) {
    return drain_impl(buf, cap, bytes, sum);
}

int nstack_set_rx_gro(uint32_t W) {
    if (W > RXG_GRO_MAX_WINDOW) return RXG_EINVAL;
    pthread_mutex_lock(&g_lock);
    /* (payloads left in their frames; assembled streams are coalesced already) */
    int rc = W && (g_inplace || g_assemble) ? RXG_EINVAL : RXG_OK;
    if (rc == RXG_OK) {
        g_gro = W;
        if (g_ctx && !g_inplace) rc = rxg_tune_deliver(g_ctx, dlv_flags());
        if (g_ctx && W && rc == RXG_OK) rc = rxg_tune_gro(g_ctx, W);
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_set_rx_inplace(int on, void (*release)(rxg_mbuf *m, void *arg), void *arg) {
    pthread_mutex_lock(&g_lock);
    if (on && (g_gro || g_assemble)) { /* (coalesced payloads and streams are gathered) */
        pthread_mutex_unlock(&g_lock);
        return RXG_EINVAL;
    }
    g_inplace = on != 0;
    g_mb_release = release;
    g_mb_arg = arg;
    const int rc = g_ctx ? rxg_tune_deliver(g_ctx, dlv_flags()) : RXG_OK;
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_set_rx_order(int on) {
    pthread_mutex_lock(&g_lock);
    g_order = on != 0;
    const int rc = g_ctx ? rxg_tune_deliver(g_ctx, dlv_flags()) : RXG_OK;
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_set_rx_assemble(int on) {
    pthread_mutex_lock(&g_lock);
    int rc = on && (g_gro || g_inplace) ? RXG_EINVAL : RXG_OK;
    if (rc == RXG_OK) {
        g_assemble = on != 0;
        if (g_ctx) rc = rxg_tune_deliver(g_ctx, dlv_flags());
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_set_rx_ddos(int on, double thresh) {
    if (thresh != thresh) return RXG_EINVAL;
    pthread_mutex_lock(&g_lock);
    g_ddos = on != 0;
    g_ddos_thresh = thresh;
    int rc = g_ctx ? rxg_tune_deliver(g_ctx, dlv_flags()) : RXG_OK;
    if (g_ctx && rc == RXG_OK) rc = rxg_tune_ddos_thresh(g_ctx, thresh);
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_ddos_status(nstack_ddos *out) {
    if (!out) return RXG_EINVAL;
    pthread_mutex_lock(&g_lock);
    *out = g_ddos_acc;
    pthread_mutex_unlock(&g_lock);
    return RXG_OK;
}

int nstack_set_syncookies(int mode, const uint8_t key[16]) {
    if (mode < 0 || mode > 2 || (mode && !key)) return RXG_EINVAL;
    pthread_mutex_lock(&g_lock);
    int rc = mode == 2 && !g_ddos ? RXG_EINVAL : RXG_OK; /* (mode 2 reads the detector's alarm) */
    if (rc == RXG_OK) {
        g_ck_mode = mode;
        if (mode) {
            uint64_t k[2] = {0, 0};
            for (int i = 0; i < 16; i++) k[i >> 3] |= (uint64_t)key[i] << (8 * (i & 7));
            g_ck_p.k0 = k[0], g_ck_p.k1 = k[1];
            g_ck_p.max_age = RXG_CK_DEFAULT_MAX_AGE;
            g_ck_p.window = D_TCP_INITIAL_WINDOW;
            g_ck_p.t = ck_now();
        }
        if (g_ctx) rc = rxg_tune_deliver(g_ctx, dlv_flags());
        if (rc == RXG_OK) rc = ck_sync_listeners();
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_syncookie_tick(uint32_t t) {
    pthread_mutex_lock(&g_lock);
    g_ck_pin = t;
    pthread_mutex_unlock(&g_lock);
    return RXG_OK;
}

int nstack_syncookie_stats(uint64_t out[4]) {
    if (!out) return RXG_EINVAL;
    pthread_mutex_lock(&g_lock);
    out[0] = g_ck_syn, out[1] = g_ck_acc, out[2] = g_ck_rej, out[3] = 0;
    pthread_mutex_unlock(&g_lock);
    return RXG_OK;
}

void nstack_reclaim(void) { reclaim(); }

void nstack_mbufs_put(rxg_mbuf *const *m, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (m[i]) mb_put(m[i]);
}

int nstack_flow_ids(uint32_t *uid, uint32_t cap_u, uint32_t *tid, uint32_t cap_t) {
    pthread_mutex_lock(&g_lock);
    int rc = g_ctx ? RXG_OK : RXG_EINVAL;
    if (rc == RXG_OK && g_dirty) rc = snapshot();
    if (rc == RXG_OK) {
        if (uid) memcpy(uid, s_udp_id, (size_t)(s_nu < cap_u ? s_nu : cap_u) * sizeof(*uid));
        if (tid) memcpy(tid, s_tcb_id, (size_t)(s_nt < cap_t ? s_nt : cap_t) * sizeof(*tid));
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

rxg_ctx *nstack_ctx(void) { return g_ctx; }

int nstack_register_host(void *base, uint64_t bytes) {
    pthread_mutex_lock(&g_lock);
    const int rc = g_ctx ? rxg_register_host(g_ctx, base, bytes) : RXG_EINVAL;
    pthread_mutex_unlock(&g_lock);
    return rc;
}

uint32_t nstack_lookup_udp(uint32_t dip, uint16_t dport) {
    pthread_mutex_lock(&g_lock);
    const uint32_t f = g_ctx ? rxg_ft_lookup_udp(g_ctx, dip, dport) : RXG_FLOW_NONE;
    pthread_mutex_unlock(&g_lock);
    return f;
}

uint32_t nstack_lookup_tcp(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport) {
    pthread_mutex_lock(&g_lock);
    const uint32_t f = g_ctx ? rxg_ft_lookup_tcp(g_ctx, sip, dip, sport, dport) : RXG_FLOW_NONE;
    pthread_mutex_unlock(&g_lock);
    return f;
}

/* ---- TX: one udp_out + tcp_out pass of the protocol loop (netfamily.c:205-206) */
static inline void wr16be(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}
static inline void wr32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }

/* ng_encode_arp_pkt, common.c:206-241 (request, opcode 1); an all-ones
 * target MAC puts the zero MAC into the Ethernet destination (:216-223) */
static uint32_t enc_arp(uint8_t *m, const uint8_t *dst_mac, uint32_t sip, uint32_t dip) {
    static const uint8_t zero[6];
    memcpy(m, memcmp(dst_mac, k_default_arp_mac, 6) ? dst_mac : zero, 6);
    memcpy(m + 6, g_local_mac, 6);
    wr16be(m + 12, 0x0806);
    wr16be(m + 14, 1);
    wr16be(m + 16, 0x0800);
    m[18] = 6;
    m[19] = 4;
    wr16be(m + 20, 1);
    memcpy(m + 22, g_local_mac, 6);
    wr32(m + 28, sip);
    memcpy(m + 32, dst_mac, 6);
    wr32(m + 38, dip);
    return 42;
}

/* IPv4 header of ng_encode_udp_apppkt / ng_encode_tcp_apppkt (udp.c:74-85,
 * tcp.c:434-445); the header checksum is left 0 for rxg_tx_cksum */
static void enc_ipv4(uint8_t *ip, uint32_t total_len, uint8_t proto, uint32_t sip, uint32_t dip) {
    ip[0] = 0x45;
    ip[1] = 0;
    wr16be(ip + 2, total_len - 14);
    wr16be(ip + 4, 0);
    wr16be(ip + 6, 0);
    ip[8] = 64;
    ip[9] = proto;
    ip[10] = ip[11] = 0;
    wr32(ip + 12, sip);
    wr32(ip + 16, dip);
}

/* ng_encode_udp_apppkt, udp.c:59-98: total = length + 42 */
static uint32_t enc_udp(uint8_t *m, const uint8_t *src_mac, const uint8_t *dst_mac,
                        const struct offload *o) {
    const uint32_t total = (uint32_t)o->length + 42u;
    memcpy(m, dst_mac, 6);
    memcpy(m + 6, src_mac, 6);
    wr16be(m + 12, 0x0800);
    enc_ipv4(m + 14, total, IPPROTO_UDP, o->sip, o->dip);
    memcpy(m + 34, &o->sport, 2);
    memcpy(m + 36, &o->dport, 2);
    wr16be(m + 38, total - 34); /* dgram_len = 8 + payload (udp.c:91-92) */
    m[40] = m[41] = 0;
    if (o->length) memcpy(m + 42, o->data, o->length);
    return total;
}

/* ng_encode_tcp_apppkt, tcp.c:420-466: total = 54 + 4*optlen + length; the
 * window is stored without htons (tcp.c:454), options are not written (0) */
static uint32_t enc_tcp(uint8_t *m, const uint8_t *src_mac, const uint8_t *dst_mac, uint32_t sip,
                        uint32_t dip, const struct tcp_fragment *f) {
    const uint32_t opt = (uint32_t)f->optlen * 4u, total = 54u + opt + f->length;
    memcpy(m, dst_mac, 6);
    memcpy(m + 6, src_mac, 6);
    wr16be(m + 12, 0x0800);
    enc_ipv4(m + 14, total, IPPROTO_TCP, sip, dip);
    uint8_t *t = m + 34;
    memcpy(t, &f->sport, 2);
    memcpy(t + 2, &f->dport, 2);
    wr32(t + 4, htonl(f->seqnum));
    wr32(t + 8, htonl(f->acknum));
    t[12] = f->hdrlen_off;
    t[13] = f->tcp_flags;
    memcpy(t + 14, &f->windows, 2);
    t[16] = t[17] = 0;
    memcpy(t + 18, &f->tcp_urp, 2);
    memset(t + 20, 0, opt);
    if (f->data && f->length) memcpy(t + 20 + opt, f->data, f->length);
    return total;
}

static inline uint64_t align64(uint64_t x) { return (x + 63u) & ~63ull; }

int nstack_set_local(uint32_t ip, const uint8_t mac[6]) {
    pthread_mutex_lock(&g_lock);
    g_local_ip = ip;
    if (mac) memcpy(g_local_mac, mac, 6);
    (void)l2_sync(); /* (the responder answers for the address of its next burst) */
    pthread_mutex_unlock(&g_lock);
    return 0;
}

int nstack_set_l2_respond(int on) {
    pthread_mutex_lock(&g_lock);
    int rc = on && !g_local_ip ? RXG_EINVAL : RXG_OK;
    if (rc == RXG_OK) {
        g_l2 = on != 0;
        if (g_ctx) rc = rxg_tune_deliver(g_ctx, dlv_flags());
        if (rc == RXG_OK) rc = l2_sync();
    }
    pthread_mutex_unlock(&g_lock);
    return rc;
}

int nstack_arp_insert(uint32_t ip, const uint8_t mac[6]) {
    if (!mac) return RXG_EINVAL;
    pthread_mutex_lock(&g_lock);
    int r = arp_insert(ip, mac);
    pthread_mutex_unlock(&g_lock);
    return r;
}

static void tx_place(uint8_t *fp, uint32_t fl, uint64_t *pos, uint32_t *off, uint16_t *len,
                     uint32_t *n);

/* ---- TX through the GPU encoder (K5, nstack_set_tx_encode): the walks of
 * nstack_tx_burst fill send descriptors instead of frames, the payloads go
 * into a staging buffer (pinned through rxg_register_host where the context
 * has a device) at 16-B aligned offsets, and one rxg_tx_encode call writes the
 * burst.  Used by the protocol thread only. */
static int g_tx_encode;
static atomic_ullong g_txe_frames; /* stat 13 */
static rxg_txd *s_txd;
static uint32_t s_txd_cap;
static uint8_t *s_txpay;
static uint64_t s_txpay_cap, s_txpay_len;
/* TCP segmentation (nstack_set_tx_mss): tcp_out's walk sends a fragment longer
 * than the MSS as several frames; 0 = off */
static uint32_t g_tx_mss;
static atomic_ullong g_tso_frags; /* stat 14 */
static uint32_t *s_txseg;         /* rxg_tx_encode_tso's first / nseg */
static uint32_t s_txseg_cap;
/* IPv4 fragmentation (nstack_set_tx_mtu): udp_out's walk sends a datagram that
 * does not fit the MTU as its fragments; 0 = off.  The id of the next cut
 * datagram: 1 after init or fini */
static uint32_t g_tx_mtu;
static uint16_t g_ip_id = 1;
static atomic_ullong g_udp_frags; /* stat 25 */

int nstack_set_tx_mtu(uint32_t mtu) {
    if (mtu && (mtu < 68u || mtu > 65535u)) return RXG_EINVAL;
    pthread_mutex_lock(&g_lock);
    g_tx_mtu = mtu;
    pthread_mutex_unlock(&g_lock);
    return 0;
}

static uint32_t raw_sum16(const uint8_t *p, uint32_t n, uint32_t s) {
    uint32_t i = 0;
    for (; i + 1 < n; i += 2) s += (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8);
    if (i < n) s += p[i];
    return s;
}
static uint16_t fold_not16(uint32_t s) {
    s = (s >> 16) + (s & 0xFFFFu);
    s = (s >> 16) + (s & 0xFFFFu);
    return (uint16_t)~s;
}

/* the s fragments of datagram o (fp datagram bytes each, include/rxgpu.h) from
 * *pos on; cksum: every header checksum and the datagram's UDP checksum filled
 * here (rxg_tx_cksum knows whole datagrams only) */
static void enc_udp_frags(uint8_t *pkts, const uint8_t *src_mac, const uint8_t *dst_mac,
                          const struct offload *o, uint32_t fp, uint32_t s, uint16_t id, int cksum,
                          uint64_t *pos, uint32_t *off, uint16_t *len, uint32_t *n) {
    const uint32_t L = 8u + (uint32_t)o->length;
    uint16_t k16 = 0;
    if (cksum) { /* rte_ipv4_udptcp_cksum over the whole datagram, 0 -> 0xFFFF */
        uint8_t h[20];
        wr32(h, o->sip), wr32(h + 4, o->dip);
        h[8] = 0, h[9] = IPPROTO_UDP;
        wr16be(h + 10, L);
        memcpy(h + 12, &o->sport, 2), memcpy(h + 14, &o->dport, 2);
        wr16be(h + 16, L);
        h[18] = h[19] = 0;
        k16 = fold_not16(raw_sum16(o->data, o->length, raw_sum16(h, 20, 0)));
        if (!k16) k16 = 0xFFFF;
    }
    for (uint32_t j = 0; j < s; j++) {
        const uint32_t at = j * fp, b = j + 1 == s ? L - at : fp, fl = 34u + b;
        uint8_t *m = pkts + *pos;
        memcpy(m, dst_mac, 6);
        memcpy(m + 6, src_mac, 6);
        wr16be(m + 12, 0x0800);
        enc_ipv4(m + 14, fl, IPPROTO_UDP, o->sip, o->dip);
        wr16be(m + 18, id);
        wr16be(m + 20, (at >> 3) | (j + 1 < s ? 0x2000u : 0u));
        if (cksum) {
            const uint16_t hip = fold_not16(raw_sum16(m + 14, 20, 0)); /* the plain complement */
            memcpy(m + 24, &hip, 2);
        }
        uint32_t done = 0;
        if (j == 0) {
            memcpy(m + 34, &o->sport, 2);
            memcpy(m + 36, &o->dport, 2);
            wr16be(m + 38, L);
            memcpy(m + 40, &k16, 2);
            done = 8;
        }
        if (b > done) memcpy(m + 34 + done, o->data + (at + done - 8u), b - done);
        tx_place(m, fl, pos, off, len, n);
    }
}

int nstack_set_tx_mss(uint32_t mss) {
    if (mss & 3u) return RXG_EINVAL;
    pthread_mutex_lock(&g_lock);
    g_tx_mss = mss;
    pthread_mutex_unlock(&g_lock);
    return 0;
}

int nstack_set_tx_encode(int on) {
    pthread_mutex_lock(&g_lock);
    g_tx_encode = on != 0;
    pthread_mutex_unlock(&g_lock);
    return 0;
}

static void tx_stage_free(void) {
    if (s_txpay && g_ctx) (void)rxg_unregister_host(g_ctx, s_txpay);
    free(s_txpay), free(s_txd), free(s_txseg);
    s_txpay = NULL, s_txd = NULL, s_txseg = NULL;
    s_txpay_cap = s_txpay_len = 0;
    s_txd_cap = s_txseg_cap = 0;
}

/* room for `bytes` more staged payload bytes (to their 16-B end); 0 = no memory */
static int tx_stage_room(uint64_t bytes) {
    const uint64_t need = s_txpay_len + ((bytes + 15u) & ~15ull);
    if (need <= s_txpay_cap) return 1;
    uint64_t cap = s_txpay_cap ? s_txpay_cap : 1u << 16;
    while (cap < need) cap *= 2;
    void *p = NULL;
    if (posix_memalign(&p, 4096, cap)) return 0;
    if (s_txpay_len) memcpy(p, s_txpay, s_txpay_len);
    if (s_txpay && g_ctx) (void)rxg_unregister_host(g_ctx, s_txpay);
    free(s_txpay);
    s_txpay = p;
    s_txpay_cap = cap;
    if (g_ctx) (void)rxg_register_host(g_ctx, p, cap); /* pinned where there is a device */
    return 1;
}

/* descriptor *nd of the burst: its payload staged (the caller has made room),
 * the position advanced by its frames' `bytes` as tx_place does; kind
 * RXG_TXD_ARP: ng_send_arp's request for dip (enc_arp) */
static void tx_describe(uint32_t kind, const uint8_t *src_mac, const uint8_t *dst_mac, uint32_t sip,
                        uint32_t dip, const struct tcp_fragment *f, uint16_t sport, uint16_t dport,
                        const uint8_t *data, uint32_t length, uint64_t bytes, uint64_t *pos,
                        uint32_t *nd) {
    rxg_txd *d = &s_txd[*nd];
    memset(d, 0, sizeof(*d));
    memcpy(d->dst_mac, dst_mac, 6);
    memcpy(d->src_mac, src_mac, 6);
    d->sip = sip, d->dip = dip;
    d->sport = sport, d->dport = dport;
    d->kind = (uint8_t)kind;
    if (f) {
        d->seq = f->seqnum, d->ack = f->acknum;
        d->window = f->windows, d->urp = f->tcp_urp;
        d->hdrlen_off = f->hdrlen_off, d->tcp_flags = f->tcp_flags;
        d->optlen = (uint8_t)f->optlen;
    }
    d->pay_off16 = (uint32_t)(s_txpay_len >> 4);
    d->pay_len = length;
    if (length) {
        if (data) memcpy(s_txpay + s_txpay_len, data, length);
        else memset(s_txpay + s_txpay_len, 0, length);
        s_txpay_len += ((uint64_t)length + 15u) & ~15ull;
    }
    *pos += bytes;
    ++*nd;
}

/* frame k of the burst: zero fill to the 64-B slot end, descriptor */
static void tx_place(uint8_t *fp, uint32_t fl, uint64_t *pos, uint32_t *off, uint16_t *len,
                     uint32_t *n) {
    memset(fp + fl, 0, align64(fl) - fl);
    off[*n] = (uint32_t)(*pos >> 6);
    len[*n] = (uint16_t)fl;
    *pos += align64(fl);
    ++*n;
}

int nstack_tx_burst(uint8_t *pkts, uint64_t cap_bytes, uint32_t *off, uint16_t *len,
                    uint32_t max_frames, int cksum, uint64_t *span) {
    if (span) *span = 0;
    if (!pkts || !off || !len) return max_frames ? RXG_EINVAL : 0;
    reclaim();
    proto_lock();
    uint32_t n = 0, nd = 0; /* frames; the encoder's descriptors */
    uint64_t pos = 0;
    int full = 0;
    const uint32_t mss = g_tx_mss, mtu = g_tx_mtu;
    uint32_t nfrag = 0; /* host-framed fragments: complete frames, not rxg_tx_cksum's */
    /* the GPU encoder: descriptors instead of frames (same walks, same rules) */
    int enc = g_tx_encode && cksum && max_frames;
    if (enc) {
        s_txpay_len = 0;
        if (s_txd_cap < max_frames) {
            rxg_txd *t = realloc(s_txd, (size_t)max_frames * sizeof(*t));
            if (!t) {
                pthread_mutex_unlock(&g_lock);
                return RXG_ENOMEM;
            }
            s_txd = t, s_txd_cap = max_frames;
        }
        if ((mss || mtu) && s_txseg_cap < max_frames) {
            uint32_t *t = realloc(s_txseg, (size_t)max_frames * 2 * sizeof(*t));
            if (!t) {
                pthread_mutex_unlock(&g_lock);
                return RXG_ENOMEM;
            }
            s_txseg = t, s_txseg_cap = max_frames;
        }
    }
    /* the L2 responder's answers first, oldest first: complete frames, copied
     * as they are; the walks below (and the encoder) get the room and the
     * frame slots behind them */
    while (g_l2q_n && n < max_frames && !full) {
        struct l2_ans *a = &s_l2q[g_l2q_head];
        if (pos + align64(a->len) > cap_bytes) {
            full = 1;
            break;
        }
        uint8_t *fp = pkts + pos;
        memcpy(fp, a->b, a->len);
        tx_place(fp, a->len, &pos, off, len, &n);
        g_l2q_bytes -= align64(a->len);
        free(a->b);
        a->b = NULL;
        g_l2q_head = (g_l2q_head + 1) % L2_Q_FRAMES, g_l2q_n--;
    }
    const uint32_t n0 = n;
    const uint64_t pos0 = pos;
    /* udp_out, udp.c:123-164: at most one datagram per socket, list order */
    for (struct localhost *h = g_pstHost; h && n < max_frames && !full; h = h->next) {
        struct offload *o = NULL;
        pthread_mutex_lock(&h->mutex);
        if (ring_peek(h->sndbuf, (void **)&o) != 0) {
            pthread_mutex_unlock(&h->mutex);
            continue;
        }
        const uint8_t *dmac = arp_lookup(o->dip);
        if (dmac && mtu && 28ull + o->length > mtu) {
            /* cut at the MTU: its s fragments go out now, all or none */
            const uint32_t L = 8u + (uint32_t)o->length, fp = (mtu - 20u) & ~7u;
            const uint32_t s = (L + fp - 1u) / fp;
            const uint64_t bytes = (uint64_t)(s - 1u) * align64(34u + fp) +
                                   align64(34u + (L - (s - 1u) * fp));
            if (28ull + o->length > 65535u || 34u + fp > 65535u || s > max_frames ||
                bytes > cap_bytes) { /* no pass of this size can carry it: dropped */
                ring_dequeue(h->sndbuf, (void **)&o);
                pthread_mutex_unlock(&h->mutex);
                free(o->data);
                free(o);
                g_stat[1]++;
                continue;
            }
            if (n + s > max_frames || pos + bytes > cap_bytes || (enc && !tx_stage_room(o->length))) {
                pthread_mutex_unlock(&h->mutex);
                full = 1;
                break;
            }
            ring_dequeue(h->sndbuf, (void **)&o);
            pthread_mutex_unlock(&h->mutex);
            const uint16_t id = g_ip_id++;
            if (enc) { /* one descriptor: the encoder cuts it the same way */
                tx_describe(RXG_TXD_UDP, h->localmac, dmac, o->sip, o->dip, NULL, o->sport, o->dport,
                            o->data, o->length, bytes, &pos, &nd);
                s_txd[nd - 1].seq = id;
                n += s;
            } else {
                enc_udp_frags(pkts, h->localmac, dmac, o, fp, s, id, cksum, &pos, off, len, &n);
                nfrag += s;
            }
            atomic_fetch_add_explicit(&g_udp_frags, 1, memory_order_relaxed);
            free(o->data);
            free(o);
            continue;
        }
        const uint32_t fl = dmac ? 42u + o->length : 42u;
        if (fl > 65535u) { /* no frame can carry it: dropped */
            ring_dequeue(h->sndbuf, (void **)&o);
            pthread_mutex_unlock(&h->mutex);
            free(o->data);
            free(o);
            g_stat[1]++;
            continue;
        }
        if (pos + align64(fl) > cap_bytes || (enc && !tx_stage_room(dmac ? o->length : 0))) {
            pthread_mutex_unlock(&h->mutex);
            full = 1;
            break;
        }
        ring_dequeue(h->sndbuf, (void **)&o);
        uint8_t *fp = pkts + pos;
        if (!dmac) { /* an ARP request first, the datagram queued again (udp.c:139-146) */
            if (enc)
                tx_describe(RXG_TXD_ARP, g_local_mac, k_default_arp_mac, o->sip, o->dip, NULL, 0, 0,
                            NULL, 0, align64(fl), &pos, &nd);
            else
                enc_arp(fp, k_default_arp_mac, o->sip, o->dip);
            if (ring_enqueue(h->sndbuf, o)) {
                free(o->data);
                free(o);
                g_stat[1]++;
            }
            pthread_mutex_unlock(&h->mutex);
        } else {
            pthread_mutex_unlock(&h->mutex);
            if (enc)
                tx_describe(RXG_TXD_UDP, h->localmac, dmac, o->sip, o->dip, NULL, o->sport,
                            o->dport, o->data, o->length, align64(fl), &pos, &nd);
            else
                enc_udp(fp, h->localmac, dmac, o);
            free(o->data);
            free(o);
        }
        if (enc) n++;
        else tx_place(fp, fl, &pos, off, len, &n);
    }
    /* tcp_out, tcp.c:492-555: at most one fragment per tcb, list order */
    for (struct tcp_stream *s = g_tcb_set; s && n < max_frames && !full; s = s->next) {
        pthread_mutex_lock(&s->mutex);
        struct tcp_fragment *f = s->sndbuf ? tq_front(s->sndbuf) : NULL;
        if (!f) {
            pthread_mutex_unlock(&s->mutex);
            continue;
        }
        const uint8_t *dmac = arp_lookup(s->sip); /* the remote side (tcp.c:521) */
        /* longer than the MSS: s frames, each measured on its own */
        const int tso = dmac && mss && f->length > mss;
        const uint64_t fl64 =
            dmac ? 54u + (uint64_t)f->optlen * 4u + (tso ? mss : f->length) : 42u;
        if (fl64 > 65535u) {
            tq_pop(s->sndbuf, &s->sq);
            pthread_mutex_unlock(&s->mutex);
            g_stat[1]++;
            continue;
        }
        const uint32_t fl = (uint32_t)fl64;
        if (tso) {
            /* the r whole segments that fit max_frames and cap_bytes go out now; r < s:
             * FIN / PSH stay with the rest, which remains the head of the send queue */
            const uint32_t hdr = fl - mss;
            const uint32_t s_all = (uint32_t)(((uint64_t)f->length + mss - 1) / mss);
            uint32_t r = 0;
            uint64_t bytes = 0;
            while (r < s_all && n + r < max_frames) {
                const uint32_t sl = r + 1 == s_all ? f->length - r * mss : mss;
                if (pos + bytes + align64(hdr + sl) > cap_bytes) break;
                bytes += align64(hdr + sl);
                r++;
            }
            const uint32_t take = r == s_all ? f->length : r * mss;
            if (r == 0 || (enc && !tx_stage_room(take))) {
                pthread_mutex_unlock(&s->mutex);
                full = 1;
                break;
            }
            struct tcp_fragment g = *f;
            if (r < s_all) g.tcp_flags &= (uint8_t)~0x09u;
            if (enc) { /* one descriptor: the encoder cuts it the same way */
                tx_describe(RXG_TXD_TCP, s->localmac, dmac, s->dip, s->sip, &g, f->sport, f->dport,
                            f->data, take, bytes, &pos, &nd);
                n += r;
            } else {
                for (uint32_t j = 0; j < r; j++) {
                    g.seqnum = f->seqnum + j * mss;
                    g.data = f->data ? f->data + (size_t)j * mss : NULL;
                    g.length = j + 1 == s_all ? f->length - j * mss : mss;
                    g.tcp_flags = j + 1 == s_all ? f->tcp_flags : f->tcp_flags & (uint8_t)~0x09u;
                    uint8_t *sp = pkts + pos;
                    tx_place(sp, enc_tcp(sp, s->localmac, dmac, s->dip, s->sip, &g), &pos, off, len,
                             &n);
                }
            }
            if (r > 1) atomic_fetch_add_explicit(&g_tso_frags, 1, memory_order_relaxed);
            if (r == s_all) {
                tq_pop(s->sndbuf, &s->sq);
            } else {
                f->seqnum += take;
                f->length -= take;
                if (f->data) memmove(f->data, f->data + take, f->length);
                full = 1;
            }
            pthread_mutex_unlock(&s->mutex);
            continue;
        }
        if (pos + align64(fl) > cap_bytes || (enc && !tx_stage_room(dmac ? f->length : 0))) {
            pthread_mutex_unlock(&s->mutex);
            full = 1;
            break;
        }
        uint8_t *fp = pkts + pos;
        if (!dmac) { /* tcp.c:522-535: an ARP request, the fragment dequeued and queued again */
            if (enc)
                tx_describe(RXG_TXD_ARP, g_local_mac, k_default_arp_mac, s->dip, s->sip, NULL, 0, 0,
                            NULL, 0, align64(fl), &pos, &nd);
            else
                enc_arp(fp, k_default_arp_mac, s->dip, s->sip);
            struct tcp_fragment *d = tq_detach(s->sndbuf, &s->sq);
            if (d && tq_push(s->sndbuf, &s->sq, d)) {
                frag_item_free(d);
                g_stat[1]++;
            }
        } else {
            if (enc) /* local -> remote (tcp.c:542) */
                tx_describe(RXG_TXD_TCP, s->localmac, dmac, s->dip, s->sip, f, f->sport, f->dport,
                            f->data, f->length, align64(fl), &pos, &nd);
            else
                enc_tcp(fp, s->localmac, dmac, s->dip, s->sip, f);
            tq_pop(s->sndbuf, &s->sq);
        }
        pthread_mutex_unlock(&s->mutex);
        if (enc) n++;
        else tx_place(fp, fl, &pos, off, len, &n);
    }
    /* SYN cookies: the SYN-ACKs of the judged bursts, oldest first.  The
     * descriptor names both MACs (the SYN's, swapped): no ARP lookup */
    while (g_ck_tx_head < g_ck_tx_n && n < max_frames && !full) {
        const rxg_txd *c = &s_ck_tx[g_ck_tx_head];
        if (pos + 64u > cap_bytes) {
            full = 1;
            break;
        }
        if (enc) {
            s_txd[nd] = *c;
            s_txd[nd].pay_off16 = (uint32_t)(s_txpay_len >> 4);
            pos += 64u, nd++, n++;
        } else {
            struct tcp_fragment g;
            memset(&g, 0, sizeof(g));
            g.sport = c->sport, g.dport = c->dport;
            g.seqnum = c->seq, g.acknum = c->ack;
            g.hdrlen_off = c->hdrlen_off, g.tcp_flags = c->tcp_flags;
            g.windows = c->window, g.tcp_urp = c->urp;
            uint8_t *fp = pkts + pos;
            tx_place(fp, enc_tcp(fp, c->src_mac, c->dst_mac, c->sip, c->dip, &g), &pos, off, len, &n);
        }
        g_ck_tx_head++;
    }
    rxg_ctx *ctx = g_ctx;
    pthread_mutex_unlock(&g_lock);
    if (span) *span = pos;
    if (cksum && n > n0) { /* (the responder's answers, frames [0, n0), are complete) */
        if (!ctx) return RXG_EINVAL;
        int rc;
        const uint32_t nw = n - n0;
        if (enc) { /* K5 on the GPU: the frames, off and len of the walks' descriptors */
            uint64_t used = 0;
            if (mtu) /* nw entries from nd descriptors, both cuts */
                rc = rxg_tx_encode_frag(ctx, s_txd, nd, s_txpay, s_txpay_len, mss, mtu, pkts + pos0,
                                        cap_bytes - pos0, off + n0, len + n0, nw, s_txseg,
                                        s_txseg + max_frames, 0, &used);
            else if (mss) /* nw entries from nd descriptors */
                rc = rxg_tx_encode_tso(ctx, s_txd, nd, s_txpay, s_txpay_len, mss, pkts + pos0,
                                       cap_bytes - pos0, off + n0, len + n0, nw, s_txseg,
                                       s_txseg + max_frames, 0, &used);
            else
                rc = rxg_tx_encode(ctx, s_txd, nw, s_txpay, s_txpay_len, pkts + pos0, cap_bytes - pos0,
                                   off + n0, len + n0, 0, &used);
            for (uint32_t k = n0; pos0 && k < n; k++) off[k] += (uint32_t)(pos0 >> 6);
            if (rc == RXG_OK && used != pos - pos0) rc = RXG_ERANGE;
            if (rc == RXG_OK) atomic_fetch_add_explicit(&g_txe_frames, nw, memory_order_relaxed);
        } else if (nfrag) { /* K2 on the frames that are whole datagrams */
            uint32_t *xo = malloc((size_t)nw * (sizeof(*xo) + sizeof(uint16_t)));
            if (!xo) return RXG_ENOMEM;
            uint16_t *xl = (uint16_t *)(xo + nw);
            uint32_t m = 0;
            for (uint32_t k = n0; k < n; k++) {
                const uint8_t *f = pkts + ((uint64_t)off[k] << 6);
                if (len[k] >= 34 && f[12] == 0x08 && f[13] == 0x00 && ((f[20] & 0x3F) | f[21]))
                    continue; /* a fragment: filled by enc_udp_frags */
                xo[m] = off[k], xl[m] = len[k], m++;
            }
            rc = m ? rxg_tx_cksum(ctx, pkts, pos, xo, xl, m, 6) : RXG_OK;
            free(xo);
        } else {
            rc = rxg_tx_cksum(ctx, pkts, pos, off + n0, len + n0, nw, 6); /* K2 on the GPU */
        }
        if (rc) return rc;
    }
    return (int)n;
}

uint64_t nstack_stat(int which) {
    if (which < 0 || which > 25) return 0;
    if (which == 25) return (uint64_t)atomic_load_explicit(&g_udp_frags, memory_order_relaxed);
    if (which >= 21) { /* the L2 responder: ARP / echo answers queued, answers dropped for
                          room, echo requests with a bad checksum or a cut capture */
        pthread_mutex_lock(&g_lock);
        const uint64_t a = which == 21 ? g_l2_arp : which == 22 ? g_l2_echo : which == 23 ? g_l2_drop : g_l2_bad;
        pthread_mutex_unlock(&g_lock);
        return a;
    }
    if (which >= 15) { /* segments absorbed by receive coalescing / moved by ordering; the
                          flood detector's frames under alarm / rises; stream assembly's
                          bytes already received / streams behind a hole */
        pthread_mutex_lock(&g_lock);
        const uint64_t a = which == 15   ? g_gro_absorbed
                           : which == 16 ? g_order_moved
                           : which == 17 ? g_ddos_acc.alarm_frames
                           : which == 18 ? g_ddos_acc.rises
                           : which == 19 ? g_asm_dup
                                         : g_asm_hole;
        pthread_mutex_unlock(&g_lock);
        return a;
    }
    if (which == 14) return (uint64_t)atomic_load_explicit(&g_tso_frags, memory_order_relaxed);
    if (which == 13) return (uint64_t)atomic_load_explicit(&g_txe_frames, memory_order_relaxed);
    if (which == 12) return (uint64_t)atomic_load_explicit(&g_deliveries, memory_order_acquire);
    if (which == 7) return (uint64_t)atomic_load_explicit(&g_pl_batches, memory_order_relaxed);
    if (which >= 8) return (uint64_t)atomic_load_explicit(&g_drain_ns[which - 8], memory_order_relaxed);
    pthread_mutex_lock(&g_lock);
    const uint64_t v = which == 11 ? g_pl_waits
                       : which == 6 ? g_copied_bytes
                       : which == 5 ? g_stale_parts
                                    : g_stat[which];
    pthread_mutex_unlock(&g_lock);
    return v;
}
