/*
 * rxgpu.h — C ABI of the MI355X receive front end (librxgpu.so).
 *
 * Replaces the per-frame body of the reference's protocol lcore loop
 * (pkt_process, netfamily.c:152-200) and the front halves of
 *   int udp_process(struct rte_mbuf *)   udp.h:6,  udp.c:4-57
 *   int tcp_process(struct rte_mbuf *)   tcp.h:6,  tcp.c:333-371
 * together with the two flow lookups they call
 *   get_hostinfo_fromip_port(dip, port, proto)       common.c:97-108
 *   tcp_stream_search(sip, dip, sport, dport)        common.c:31-55
 * and the DPDK 19.11.12 checksum they call (rte_ip.h:121-349, inlined
 * into the reference as rte_ipv4_udptcp_cksum).
 *
 * A per-frame GPU call is meaningless, so the boundary is a BURST: the
 * caller hands over N frames (packed buffer + offsets + lengths) and gets
 * back N 16-byte verdicts that carry exactly what the reference functions
 * decide per frame (return code, matched control block, payload window,
 * checksum).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Threading: one rxg_ctx per rx thread; a context is not thread-safe.
 * Streams: bursts may run on any streams; the stream of a context's most
 * recent burst call must still exist at the context's next call (table
 * writes are ordered after it by an event recorded then).
 * Every call that touches the device switches the calling thread to the
 * context's device and back: the thread's current device is unchanged.
 * Errors: API calls return 0 or a negative RXG_E* code (rxg_strerror);
 * the library never exits the process (the reference rte_exit()s).
 */
#ifndef RXGPU_H
#define RXGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- verdict --------------------------------------------------------- */

#define RXG_FLOW_NONE 0xFFFFFFFFu

/* frame class: the branch pkt_process takes (netfamily.c:156-199) */
enum {
    RXG_CLS_ARP = 0,        /* ether_type == BE 0x0806 (then also KNI, :194-199) */
    RXG_CLS_NON_IP = 1,     /* any other non-IPv4 ether_type -> KNI (:194-199) */
    RXG_CLS_IPV4_OTHER = 2, /* IPv4, next_proto_id not 6/17 -> KNI (:188-191) */
    RXG_CLS_UDP = 3,        /* IPv4 proto 17 -> udp_process (:178-181) */
    RXG_CLS_TCP = 4         /* IPv4 proto 6  -> tcp_process (:183-186) */
};

/* per-frame return codes, identical to the reference's */
enum {
    RXG_RC_OK = 0,              /* udp.c:56 / tcp.c:417 */
    RXG_RC_TCP_BAD_CKSUM = -1,  /* tcp.c:352-357 */
    RXG_RC_TCP_NO_TCB = -2,     /* tcp.c:363-371 */
    RXG_RC_UDP_NOMEM = -2,      /* udp.c:38-43: rte_malloc(dgram_len-8) fails when
                                   dgram_len <= 8 (size 0 or wrapped size_t) */
    RXG_RC_UDP_NO_SOCKET = -3,  /* udp.c:15-19 */
    RXG_RC_KNI = 1              /* non-TCP/UDP frame handed to KNI */
};

/* verdict.flags */
#define RXG_F_TRUNC 0x01     /* the reference would read past the captured frame
                                (ip total_length or dgram_len beyond caplen): the
                                bytes past caplen are taken as zero here; the
                                reference reads adjacent memory (parity undefined) */
#define RXG_F_TCP_NEGLEN 0x02 /* TCP tl-20-hl < 0 (reference enqueues 0-length, tcp.c:157) */
#define RXG_F_UDP_SHORT 0x04  /* UDP dgram_len <= 8 (rc -2, see RXG_RC_UDP_NOMEM) */

typedef struct rxg_verdict {
    uint32_t flow_id;      /* stable id of the matched control block (UDP and TCP
                              ids are separate spaces): id i for block i of the
                              arrays given to rxg_flows_sync, or the id
                              rxg_flows_add assigned.  A removed block's id may be
                              reused by a later add.  RXG_FLOW_NONE if no match /
                              not looked up */
    uint16_t payload_off;  /* UDP: 42 (udp.c:46 copies from udp+1); TCP: 34+hl */
    uint16_t payload_len;  /* UDP: dgram_len-8 (udp.c:38); TCP: tl-20-hl (tcp.c:145-159);
                              clamped at 0 (see flags) */
    uint16_t l4_cksum;     /* rte_ipv4_udptcp_cksum with the L4 checksum field
                              taken as 0 (tcp.c:349-351); 0 for non TCP/UDP */
    uint8_t cls;           /* RXG_CLS_* */
    int8_t rc;             /* RXG_RC_* */
    uint8_t cksum_ok;      /* stored == l4_cksum (TCP verdict input; informational
                              for UDP, which the reference never verifies) */
    uint8_t flags;         /* RXG_F_* */
    uint16_t stored_cksum; /* the L4 checksum field as stored in the frame (LE u16) */
} rxg_verdict;

/* Compact 8-byte verdict (rxg_classify_dev8): the same decision in half the
 * bytes, for the device-resident burst loop, where the verdict array is a
 * quarter of the HBM traffic at 64-B frames.  It carries everything the
 * reference decides per frame (return code, matched block, payload window,
 * checksum pass/fail, class, flags); only the two checksum VALUES of the
 * 16-byte form (l4_cksum, stored_cksum) are left out — cksum_ok is their
 * comparison.  Field for field it equals rxg_verdict8_of(the 16-byte verdict). */
typedef struct rxg_verdict8 {
    uint32_t flow_id;     /* = rxg_verdict.flow_id */
    uint16_t payload_len; /* = rxg_verdict.payload_len */
    uint8_t off_neg;      /* bits 0-6: payload_off (0, 42 or 34 + 4*hl <= 94);
                             bit 7: RXG_F_TCP_NEGLEN */
    uint8_t status;       /* bits 0-2: cls; bits 3-5: rc (3-bit two's complement);
                             bit 6: cksum_ok; bit 7: RXG_F_TRUNC */
} rxg_verdict8;

#define RXG_V8_PAYLOAD_OFF(v) ((uint32_t)((v).off_neg & 0x7Fu))
#define RXG_V8_CLS(v) ((uint32_t)((v).status & 7u))
#define RXG_V8_RC(v) ((int32_t)(((v).status >> 3) & 7u) - (int32_t)((((v).status >> 3) & 4u) << 1))
#define RXG_V8_CKSUM_OK(v) ((uint32_t)(((v).status >> 6) & 1u))
/* RXG_F_* of the 16-byte form (UDP_SHORT: a UDP frame with payload_len 0) */
#define RXG_V8_FLAGS(v)                                                                 \
    ((uint32_t)((v).status >> 7) | ((uint32_t)((v).off_neg >> 7) << 1) |              \
     ((RXG_V8_CLS(v) == RXG_CLS_UDP && (v).payload_len == 0) ? (uint32_t)RXG_F_UDP_SHORT : 0u))

static inline rxg_verdict8 rxg_verdict8_of(const rxg_verdict *v) {
    rxg_verdict8 r;
    r.flow_id = v->flow_id;
    r.payload_len = v->payload_len;
    r.off_neg = (uint8_t)((v->payload_off & 0x7Fu) | ((v->flags & RXG_F_TCP_NEGLEN) ? 0x80u : 0u));
    r.status = (uint8_t)((v->cls & 7u) | (((uint32_t)(uint8_t)v->rc & 7u) << 3) |
                         ((v->cksum_ok & 1u) << 6) | ((v->flags & RXG_F_TRUNC) ? 0x80u : 0u));
    return r;
}

/* ---- control-block snapshot (flow table source) ---------------------- */

/* One UDP socket = one `struct localhost` of the reference (udp.h:10-29).
 * Fields are raw network-order values exactly as the reference stores them
 * (nbind, common.c:350-353). */
typedef struct rxg_udp_sock {
    uint32_t localip;
    uint16_t localport;
    uint8_t protocol; /* IPPROTO_UDP for every socket nsocket() makes */
    uint8_t _pad;
} rxg_udp_sock;

/* One `struct tcp_stream` (tcp.h:29-55): key fields + status. sip/sport are
 * the remote side as read from the packet (tcp_stream_create, tcp.c:16-19). */
typedef struct rxg_tcb {
    uint32_t sip;
    uint32_t dip;
    uint16_t sport;
    uint16_t dport;
    uint32_t status; /* TCP_STATUS_* of tcp.h:10-26; LISTEN == 1 */
} rxg_tcb;

#define RXG_TCP_STATUS_LISTEN 1u

/* ---- mbuf-shaped descriptor (rte_mbuf field offsets, DPDK 19.11) ------- */
typedef struct rxg_mbuf {
    void *buf_addr;        /* @0  */
    uint8_t _r0[8];
    uint16_t data_off;     /* @16 */
    uint16_t refcnt;       /* @18: references (rte_mbuf_refcnt); librxgpu never reads it,
                              libnstack's in-place delivery holds frames with it */
    uint8_t _r1[20];
    uint16_t data_len;     /* @40 */
    uint8_t _r2[86];
} rxg_mbuf;                /* 128 bytes, like rte_mbuf */

/* ---- error codes ------------------------------------------------------ */
enum {
    RXG_OK = 0,
    RXG_EINVAL = -22,
    RXG_ENOMEM = -12,
    RXG_ENODEV = -19,
    RXG_ERANGE = -34,
    RXG_EHIP = -1000, /* HIP runtime error (details: rxg_last_hip_error) */
    RXG_ECOMM = -1001 /* RCCL error (details: rxg_last_hip_error) */
};

typedef struct rxg_ctx rxg_ctx;

/* device argument of rxg_open for a control-plane-only context: flow tables
 * and host lookups work, every burst call returns RXG_ENODEV */
#define RXG_HOST_ONLY (-1)

/* Open a context on HIP device `device`. max_pkts / max_bytes size the pinned
 * host staging and device buffers used by rxg_classify (host-buffer path);
 * rxg_classify_dev needs neither. */
int rxg_open(rxg_ctx **ctx, int device, uint32_t max_pkts, uint64_t max_bytes);
void rxg_close(rxg_ctx *ctx);
const char *rxg_strerror(int err);
const char *rxg_last_hip_error(void);

/* Mirror of the reference's control-block lists, given in CREATION order
 * (oldest first = the reverse of the head-inserted list, common.h:43-49), so
 * that on duplicate keys the highest index (the newest block) wins exactly as
 * the reference's first-match list scan does.  Builds the device flow tables
 * (linear-probed exact keys under the context's random hash seed, direct
 * port tables for listeners and UDP sockets).  Blocking: waits for this
 * context's own bursts still reading the old tables (never for other work on
 * the device), uploads, and returns with the tables in place. */
int rxg_flows_sync(rxg_ctx *ctx, const rxg_udp_sock *u, uint32_t nu, const rxg_tcb *t,
                   uint32_t nt);

/* Incremental control-block changes, between bursts.  The reference creates
 * a tcb on every SYN (tcp_stream_create + LL_ADD, tcp.c:3-52), creates and
 * binds sockets (nsocket / nbind / nlisten, common.c:262-386) and frees
 * blocks on the last ACK and on close (tcp.c:321, common.c:620,660); these
 * calls mirror exactly that on the context's tables in O(1) host work each,
 * instead of a rebuild through rxg_flows_sync.
 *
 * Flow ids are stable: rxg_flows_sync gives block i of its arrays id i; an
 * added block gets a free id (freed ids are reused, else the id space grows)
 * and keeps it until removed.  Verdicts name blocks by these ids, and the
 * per-flow counts are laid out as UDP ids [0, rxg_num_udp_ids()) followed by
 * TCP ids (count index rxg_num_udp_ids() + id); rxg_num_flows() = the length.
 * An added block is the NEWEST (it wins duplicate keys, as LL_ADD's head
 * insert makes it); an update keeps the block's creation order (nbind and
 * nlisten do not move a block in the list) and changes its key and/or
 * status; removing the newest of a duplicate key exposes the next older one.
 *
 * Changes are host-side until committed: rxg_flows_commit(stream), or
 * implicitly by the next burst call, on that burst's stream.  A commit writes
 * only the changed table slots (a small kernel on `stream`), ordered after
 * every earlier burst of this context on any stream and before every later
 * one: it never synchronises the device or the host (a table past load 1/2,
 * or a probe sequence past the cap, is rebuilt whole: that commit waits for
 * its host-to-device copies).
 *
 * rxg_flows_add returns 1 (not an error) when it grew the UDP id space, i.e.
 * moved the TCP count indices: callers keeping their own d_counts vectors
 * re-size them to rxg_num_flows(); the context's own counts move by themselves. */
int rxg_flows_add(rxg_ctx *ctx, const rxg_udp_sock *u, uint32_t nu, const rxg_tcb *t, uint32_t nt,
                  uint32_t *udp_ids, uint32_t *tcp_ids);
int rxg_flows_remove(rxg_ctx *ctx, const uint32_t *udp_ids, uint32_t nu, const uint32_t *tcp_ids,
                     uint32_t nt);
int rxg_flows_update_udp(rxg_ctx *ctx, uint32_t id, const rxg_udp_sock *u);
int rxg_flows_update_tcb(rxg_ctx *ctx, uint32_t id, const rxg_tcb *t);
int rxg_flows_commit(rxg_ctx *ctx, void *stream);
/* UDP part of the count layout (see above) */
uint32_t rxg_num_udp_ids(const rxg_ctx *ctx);
/* whole-table rebuilds so far (growth, reseeds): diagnostics */
uint32_t rxg_flows_rebuilds(const rxg_ctx *ctx);

/* Device-resident burst: all pointers are device pointers.  Frame i starts at
 * d_pkts + (d_off[i] << off_unit_log2) (off_unit_log2 >= 4: 16-byte aligned
 * starts) and has d_len[i] captured bytes; the buffer must extend to the next
 * 16-byte boundary after every frame.  len_hint = typical frame length (picks
 * lanes per frame; 0 = 1518).  If d_counts != NULL, per-flow packet counts are
 * added into it (u64[nu + nt]: UDP flows first, then TCP).  Asynchronous on
 * `stream` (a hipStream_t; NULL = the null stream). */
int rxg_classify_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                     const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                     uint32_t len_hint, rxg_verdict *d_out, uint64_t *d_counts,
                     void *stream);

/* rxg_classify_dev with the per-flow counts on a second stream: the verdicts
 * are written on `stream` as above; d_counts is complete once `count_stream`
 * (ordered after this burst's classify) has reached this point, not `stream`.
 * Above 8192 flows the counts are two passes after the classify kernel
 * (DESIGN.md §4); on count_stream they overlap the NEXT burst's classify on
 * `stream` (the context double-buffers its count indices), which is how a
 * burst loop hides them.  The caller orders readers of d_counts (a copy, the
 * RCCL all-reduce) after count_stream.  count_stream NULL or == stream: same
 * as rxg_classify_dev.  Replaces no reference call: the reference keeps no
 * per-flow counters; this is the statistic the multi-GPU path all-reduces. */
int rxg_classify_dev_cs(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                        const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                        uint32_t len_hint, rxg_verdict *d_out, uint64_t *d_counts,
                        void *stream, void *count_stream);

/* rxg_classify_dev_cs writing compact 8-byte verdicts (d_out: n x 8 bytes,
 * 8-byte aligned); kernels, counts and streams exactly as there. */
int rxg_classify_dev8(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                      const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                      uint32_t len_hint, rxg_verdict8 *d_out, uint64_t *d_counts, void *stream,
                      void *count_stream);

/* Host-buffer burst (PCIe-inclusive): copies frames + descriptors to the
 * device, classifies, copies verdicts back, accumulates the context's own
 * per-flow counts.  Synchronous. */
int rxg_classify(rxg_ctx *ctx, const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                 uint32_t n, uint32_t off_unit_log2, rxg_verdict *out);

/* Same, with the caller stating how many bytes of `pkts` the burst spans
 * (every frame end <= span_bytes); skips the O(n) scan rxg_classify makes. */
int rxg_classify_span(rxg_ctx *ctx, const uint8_t *pkts, uint64_t span_bytes, const uint32_t *off,
                      const uint16_t *len, uint32_t n, uint32_t off_unit_log2, rxg_verdict *out);

/* The reference's calling convention: a burst of mbuf pointers as dequeued at
 * netfamily.c:147.  Frames are gathered into the context's staging buffer. */
int rxg_process_mbufs(rxg_ctx *ctx, rxg_mbuf *const *m, uint32_t n, rxg_verdict *out);

/* Register host memory that holds frames — the mbuf pool's memory, as DPDK
 * hands it out (rte_mempool_mem_iter) — with the context: it is pinned and
 * mapped for the device once, and from then on an mbuf burst
 * (rxg_process_mbufs*) whose frames all lie in registered memory, 16-B
 * aligned with their 16-B rounded ends inside it, is pulled by the device
 * straight from that memory over PCIe (the DMA a NIC does into its ring)
 * instead of being gathered into pinned staging by a host memcpy and copied.
 * Other bursts take the host gather as before.  Memory registered elsewhere
 * already is accepted (and left registered at close).  Unregister waits for
 * this context's bursts. */
int rxg_register_host(rxg_ctx *ctx, void *base, uint64_t bytes);
int rxg_unregister_host(rxg_ctx *ctx, void *base);

/* Pipelined host-buffer bursts (PCIe-inclusive, overlapped).  The context owns
 * RXG_PIPE_DEPTH staging slots (each sized by rxg_open's max_pkts/max_bytes);
 * burst t copies in while burst t-1 is classified and burst t-2's verdicts
 * copy out.  rxg_submit returns at once with a ticket; the caller keeps pkts,
 * off, len and out untouched until rxg_wait(ticket) returns (pass pinned host
 * memory, e.g. hipHostMalloc'd or hipHostRegister'ed, or the copies are not
 * asynchronous).  Tickets complete in submission order.  rxg_classify_span is
 * rxg_submit + rxg_wait. */
#define RXG_PIPE_DEPTH 3
int rxg_submit(rxg_ctx *ctx, const uint8_t *pkts, uint64_t span_bytes, const uint32_t *off,
               const uint16_t *len, uint32_t n, uint32_t off_unit_log2, rxg_verdict *out,
               uint64_t *ticket);
int rxg_wait(rxg_ctx *ctx, uint64_t ticket);

/* ---- UDP delivery on the GPU: per-socket payload compaction ------------
 * The delivery half of udp_process (udp.c:25-52): for every datagram that
 * found its socket (verdict rc 0) the reference mallocs an offload, copies
 * dgram_len - 8 payload bytes from udp + 1 and enqueues it on that socket's
 * ring, frame by frame.  Here one device pass groups a classified burst's
 * delivered datagrams by socket — inside a socket in burst order, the order
 * its ring would have — and gathers their captured payload bytes into one
 * buffer, socket after socket, so the host hands each socket one contiguous
 * slice.  UDP id spaces up to RXG_COMPACT_MAX_FLOWS (the reference's socket
 * layer has at most 1024 descriptors, common.h:34). */
#define RXG_COMPACT_MAX_FLOWS 1024u
typedef struct rxg_dgram {
    uint32_t frame;  /* burst index of the datagram's frame */
    uint32_t offset; /* its payload's first byte in the compacted buffer (16-B aligned) */
    uint32_t sip;    /* raw source address (offload.sip, udp.c:31) */
    uint16_t sport;  /* raw source port (offload.sport) */
    uint16_t len;    /* payload bytes, dgram_len - 8 (udp.c:38); only the captured ones,
                        min(len, caplen - 42), are in the buffer: the rest read as 0 */
} rxg_dgram;
/* Device form, asynchronous on `stream`: d_v = the burst's verdicts; the
 * datagrams of UDP id f get ranks [d_first[f], d_first[f+1]) of d_dgram (so
 * d_first has rxg_num_udp_ids() + 1 entries, d_dgram room for n); d_totals =
 * {datagrams, payload bytes used, 1 if payload_cap was too small (those
 * payloads are not written)}.  With no UDP ids at all, d_totals[0..2] and
 * d_first[0] are cleared to 0 on `stream` and nothing else is written.
 * RXG_ERANGE above RXG_COMPACT_MAX_FLOWS ids (nothing is written). */
int rxg_udp_compact_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                        const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                        const rxg_verdict *d_v, rxg_dgram *d_dgram, uint32_t *d_first,
                        uint8_t *d_payload, uint64_t payload_cap, uint32_t *d_totals, void *stream);
/* rxg_process_mbufs followed by the compaction: verdicts into `out` as there;
 * the datagram records, the per-id first ranks and the compacted payload stay
 * in pinned buffers the context owns, valid until its next burst call
 * (*dgram: *ndgram records; *first: rxg_num_udp_ids() + 1 entries; *payload:
 * *nbytes bytes).  Synchronous. */
int rxg_process_mbufs_udp(rxg_ctx *ctx, rxg_mbuf *const *m, uint32_t n, rxg_verdict *out,
                          const rxg_dgram **dgram, const uint32_t **first, const uint8_t **payload,
                          uint32_t *ndgram, uint64_t *nbytes);

/* ---- TCP delivery on the GPU: per-connection segment sort + payload gather
 * The delivery half of tcp_process for segments that found a tcb (verdict
 * rc 0): the reference walks them frame by frame through the state machine
 * (tcp.c:373-415); an ESTABLISHED one with PSH gets a malloc'd fragment with
 * a copy of its payload (ng_tcp_enqueue_recvbuffer, tcp.c:133-185) and an ACK
 * (tcp.c:218-297).  Here one device pass sorts a classified burst's rc-0 TCP
 * segments by tcb id — stable, so a connection's segments keep burst order,
 * the order its state machine must see them in — decodes the header fields
 * the state machine reads, and gathers the payload of every PSH segment into
 * one buffer, connection after connection (each at a 16-B aligned offset), so
 * the host runs each connection's segments in order with one allocation and
 * one copy per connection per burst.  Any tcb id space. */
typedef struct rxg_segment {
    uint32_t frame;  /* burst index of the segment's frame */
    uint32_t flow;   /* tcb id (the verdict's flow_id) */
    uint32_t seq;    /* sent_seq, host order (ntohl of frame bytes 38-41) */
    uint32_t ack;    /* recv_ack, host order (ntohl of frame bytes 42-45) */
    int32_t plen;    /* total_length - 20 - 4*hl (signed: tcp.c:145-146, 391) */
    uint32_t offset; /* first payload byte in the payload buffer (16-B aligned); records
                        only (no payload buffer, RXG_DLV_TCP_IN_PLACE): the payload's
                        offset in its frame, 34 + 4*hl */
    uint16_t sport;  /* raw (network order) source port, frame bytes 34-35 */
    uint16_t dport;  /* raw destination port, frame bytes 36-37 */
    uint16_t ncopy;  /* payload bytes in the buffer: min(plen, caplen - 34 - 4*hl) for a
                        PSH segment with plen > 0, else 0; the rest of a fragment's plen
                        bytes read as 0 */
    uint8_t flags;   /* tcp_flags, frame byte 47 */
    uint8_t hl;      /* data_off >> 4, frame byte 46 */
} rxg_segment;       /* 32 bytes; bytes past the captured length read as 0 */
/* Device form, asynchronous on `stream`: d_v = the burst's verdicts; d_seg
 * (room for n) gets the rc-0 TCP segments with a tcb id below the id space,
 * sorted by (flow, frame); d_totals = {segments, payload bytes used, 1 if
 * payload_cap was too small (those payloads are not written)}.  d_payload
 * NULL: the records only (offset = the payload's offset in its frame, no
 * payload gathered).  The device
 * workspace grows on demand (stream-ordered). */
int rxg_tcp_compact_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                        const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                        const rxg_verdict *d_v, rxg_segment *d_seg, uint8_t *d_payload,
                        uint64_t payload_cap, uint32_t *d_totals, void *stream);

/* ---- TCP receive coalescing (GRO): the receive side's counterpart of TSO
 * After the sort a connection's segments are adjacent.  The coalescing form of
 * K4 recognises the in-sequence trains among them and lays each train's
 * payload down as one contiguous byte range, so the host queues one receive
 * fragment and one ACK per train instead of one per segment.  Only PSH|ACK
 * segments merge: only PSH segments deliver data here, as in the reference
 * (tcp.c:226-262), so merging never changes which bytes a connection
 * receives, only how many fragments and ACKs carry them.  The rule, on the
 * sorted records seg[0..nseg) and each record's raw source address sip (frame
 * bytes 26-29, 0 past the capture):
 *   mergeable(j): flags == 0x18 (PSH|ACK exactly), hl == 5, plen > 0 and
 *                 ncopy == plen (the payload was captured whole);
 *   j links to j-1: both mergeable; flow, sip, sport, dport and ack equal;
 *                 seq[j] == seq[j-1] + plen[j-1] (mod 2^32);
 *   a chain is a maximal range of consecutive records in which every record
 *   but the first links to its predecessor; b[j] = the 64-bit sum of plen
 *   over the chain's records before j; with the window W (bytes, 1 ..
 *   RXG_GRO_MAX_WINDOW) record j starts a new run iff it starts its chain or
 *   b[j] / W != b[j-1] / W.
 * The runs partition [0, nseg) in order; a record that is not mergeable is a
 * run of one; a run's payload is less than W + 65536 bytes.  Out-of-order
 * segments are not reordered and segments with TCP options never merge. */
typedef struct rxg_tcp_run {
    uint32_t first;  /* index of the run's first record */
    uint32_t nseg;   /* records in the run */
    uint32_t bytes;  /* sum of their ncopy */
    uint32_t offset; /* the run's start in the payload buffer (16-B aligned) */
} rxg_tcp_run;       /* 16 bytes */
#define RXG_GRO_MAX_WINDOW (1u << 20)
#define RXG_GRO_DEFAULT_WINDOW 65536u
/* rxg_tcp_compact_dev with coalescing, asynchronous on `stream`.  d_seg gets
 * field for field what rxg_tcp_compact_dev writes for the same inputs, except
 * offset: the first segment of a run sits at the run's offset and each later
 * one follows its predecessor byte-contiguously (no padding inside a run).
 * d_run (room for n) gets the runs in order, laid out one after the other,
 * each starting at the 16-B-rounded end of the one before.  d_totals (4
 * words) = {segments, payload bytes used (the 16-B-rounded end of the last
 * run), 1 if payload_cap was too small, runs}.  The bytes from a run's end to
 * its 16-B-rounded end are written as 0; a run that would pass payload_cap
 * sets the overflow flag and is not written; no other byte of d_payload is
 * touched.  d_payload is required (NULL: RXG_EINVAL), W outside 1 ..
 * RXG_GRO_MAX_WINDOW is RXG_EINVAL.  n == 0 or an empty tcb id space zeroes
 * the totals.  The device workspace grows on demand (stream-ordered). */
int rxg_tcp_coalesce_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                         const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                         const rxg_verdict *d_v, uint32_t W, rxg_segment *d_seg, rxg_tcp_run *d_run,
                         uint8_t *d_payload, uint64_t payload_cap, uint32_t *d_totals, void *stream);
/* The same rule on records in host memory (no device, no context): run (room
 * for nseg) gets the runs, offset as the device lays them out, *nrun their
 * count.  seg[].offset is neither read nor modified.  The CPU path and the
 * tests' second opinion; the device calls never fall back to it. */
int rxg_tcp_runs_host(const rxg_segment *seg, const uint32_t *sip, uint32_t nseg, uint32_t W,
                      rxg_tcp_run *run, uint32_t *nrun);

/* ---- TCP sequence ordering: the third piece beside TSO and GRO (opt-in)
 * K4's sort is stable, so a connection's segments keep their arrival order,
 * and the state machine never compares a segment's seq with rcv_nxt.  A burst
 * whose segments arrived out of order (RSS split and gather, two bursts in
 * flight, several NIC queues) therefore corrupts the byte stream.  The
 * ordering form of K4 repairs the order inside the burst: a permutation stage
 * between the sort and the record stage.  The rule, on the sorted records
 * seg[0..nseg) in (flow, frame) order and each record's raw source address
 * sip (frame bytes 26-29, 0 past the capture; rxg_tcp_runs_host's array):
 *   movable(j): (flags & 0x06) == 0, neither SYN nor RST;
 *   a group is a maximal range of consecutive movable records with equal
 *   flow, sip, sport and dport; every other record is a group of one.  Groups
 *   keep their positions and records move only inside their group: the SYNs
 *   to a listener never move relative to each other (accept order and tcb
 *   creation order are unchanged), and two sources that meet on the
 *   listener's id are never mixed;
 *   inside a group with first record h (in arrival order) let
 *   d[j] = (int32_t)(seq[j] - seq[h]); the group's records are output in
 *   ascending (d[j], j).  The cast is a bijection, so this is a total order
 *   for any input; it is the wrap-aware sequence order whenever the group
 *   spans less than 2^31 bytes.  Equal seq keeps arrival order: a pure ACK
 *   stays before the data segment that follows it, a retransmitted duplicate
 *   behind its original;
 *   moved = the number of records whose position changed.
 * A burst with no inversion comes out exactly as K4 or the coalescing form
 * writes it, with moved = 0.
 * This is reordering, not sequence validation: duplicates are not dropped,
 * nothing stops at a hole, and data of segments without PSH is still not
 * delivered (the reference's PSH-only rule).  Validation is the stream
 * assembly below ("TCP stream assembly"); this option alone does NOT make TCP
 * here loss-safe.
 *
 * One device call for both forms, asynchronous on `stream`.  W == 0:
 * rxg_tcp_compact_dev's outputs (records and gather) in the new order; d_run
 * may be NULL, and d_payload == NULL gives the records-only in-place form.
 * W in 1 .. RXG_GRO_MAX_WINDOW: rxg_tcp_coalesce_dev's outputs on the new
 * order (d_run and d_payload required).  d_totals (5 words) = {segments,
 * payload bytes used, 1 if payload_cap was too small, runs (0 when W == 0),
 * moved}.  Every other argument rule of the two calls holds.  The device
 * workspace grows on demand (stream-ordered). */
int rxg_tcp_compact_ordered_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                                const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                                const rxg_verdict *d_v, uint32_t W, rxg_segment *d_seg,
                                rxg_tcp_run *d_run, uint8_t *d_payload, uint64_t payload_cap,
                                uint32_t *d_totals, void *stream);
/* The same rule on records in host memory (no device, no context): perm[k]
 * (room for nseg) = the index of the record that takes position k, *moved the
 * count of k with perm[k] != k.  nseg == 0 is valid; a NULL argument is
 * RXG_EINVAL.  The CPU path and the tests' second opinion; the device calls
 * never fall back to it. */
int rxg_tcp_order_host(const rxg_segment *seg, const uint32_t *sip, uint32_t nseg, uint32_t *perm,
                       uint32_t *moved);

/* ---- TCP stream assembly: duplicates dropped, overlaps trimmed, a stop at
 * every hole (opt-in)
 * Ordering alone validates nothing: the state machine never compares a
 * segment's seq with rcv_nxt, so a retransmitted duplicate is delivered twice,
 * an overlapping retransmit delivers the overlap twice, a lost segment shifts
 * the byte stream, and data on a segment without PSH is dropped without being
 * counted.  After the sort and the ordering stage a connection's segments of
 * a burst are adjacent and in sequence order: which of their bytes are new is
 * a segmented running maximum, and laying them down once, contiguously, is a
 * trimmed gather.  Neither needs rcv_nxt, so the device assembles each
 * connection's burst into contiguous byte ranges ("streams") and the host,
 * which owns rcv_nxt, aligns each stream with one subtraction.
 * The rule.  Input: the records seg[0..nseg) exactly as
 * rxg_tcp_compact_ordered_dev with W = 0 orders them, each record's raw source
 * address sip (frame bytes 26-29, 0 past the capture) and avail[j], the
 * captured bytes past its TCP header: max(0, caplen - 34 - 4*hl).
 *   Groups: the ordering rule's: a maximal range of consecutive records with
 *   (flags & 0x06) == 0 and equal flow, sip, sport and dport.  A SYN or RST
 *   record is a group of one and is left alone: one stream, bytes 0, no FIN.
 *   Data length: usable(j): plen <= 0 or avail >= plen.  dlen[j] = plen if
 *   plen > 0 and usable, else 0.  Data counts with or without PSH.  A record
 *   whose payload was not captured whole contributes nothing, and its FIN is
 *   ignored.
 *   Positions, in a group with first record h (in output order):
 *     a[j] = (uint32_t)(seq[j] - seq[h]);  end[j] = a[j] + dlen[j];
 *     cov[j] = the maximum of end[i] over the group's records before j, 0 at h.
 *   All positions are 64-bit, so the rule is total for any input.
 *   New bytes: ns[j] = max(a[j], cov[j]); take[j] = end[j] - min(end[j], ns[j]);
 *   the payload bytes skipped at the front are skip[j] = dlen[j] - take[j].
 *   FIN: finok[j] = FIN set, usable and end[j] >= cov[j].
 *   Streams: record j starts a stream iff it starts its group, or
 *   a[j] > cov[j] (a hole), or finok[j-1] holds in the same group.  A stream
 *   with head p has seq = seq[h] + ns[p] (mod 2^32), bytes = the sum of take
 *   over its records, RXG_STREAM_FIN iff a finok in it (only its last record
 *   can have one), ack = the ack of its last record, first, nseg, and
 *   RXG_STREAM_HOLE when a hole started it.  Inside a stream the taken ranges
 *   are disjoint and contiguous: record j's bytes go to stream offset
 *   ns[j] - ns[p].  Where two segments carry the same byte, the one first in
 *   sequence order wins.
 *   Layout: the coalescing form's: streams in order in the payload buffer,
 *   each at the 16-B-rounded end of the one before, the pad bytes written as
 *   0; a stream that would pass payload_cap sets the overflow flag and is not
 *   written; no other byte is touched.
 * The host rule, for an ESTABLISHED tcb with rcv_nxt = R, streams in order,
 * d = (int32_t)(R - seq):
 *   d < 0: data behind a hole; nothing is delivered, one ACK with acknum R;
 *   d >= 0: fresh = bytes > d ? bytes - d : 0.  If fresh: one receive fragment
 *   of fresh bytes starting d bytes into the stream, R += fresh.  If FIN and
 *   d <= bytes: the EOF fragment, R += 1, CLOSE_WAIT (later streams are
 *   ignored).  If the stream had bytes or a FIN: snd_nxt = ack, one ACK with
 *   acknum R.  A stream with no bytes and no FIN (pure ACKs) queues nothing.
 * Over every R this delivers exactly the byte ranges, the final rcv_nxt and
 * the EOF of a sequential receiver without an out-of-order buffer that takes
 * the same records one at a time: one fragment and one ACK per connection per
 * burst, whatever the segmentation, PSH flags, duplicates or overlaps.
 * Limits: there is no reassembly queue across bursts (data behind a hole is
 * dropped and must be retransmitted), and the send side has no retransmission. */
typedef struct rxg_tcp_stream {
    uint32_t first;    /* index of the stream's first record */
    uint32_t nseg;     /* records in the stream */
    uint32_t seq;      /* sequence number of the stream's first byte */
    uint32_t ack;      /* the ack of its last record */
    uint32_t bytes;    /* new bytes: the sum of take over its records */
    uint32_t offset;   /* the stream's start in the payload buffer (16-B aligned) */
    uint32_t flags;    /* RXG_STREAM_* */
    uint32_t reserved; /* 0 */
} rxg_tcp_stream;      /* 32 bytes */
#define RXG_STREAM_FIN 0x1u
#define RXG_STREAM_HOLE 0x2u
/* Device form, asynchronous on `stream`: the sort, the ordering stage and the
 * assembly.  d_seg (room for n) gets the ordered form's records, except that
 * ncopy = take and offset = where those bytes lie in d_payload (the stream's
 * offset + ns[j] - ns[p], any byte phase).  d_stream (room for n) gets the
 * streams in order.  d_totals (6 words) = {segments, payload bytes used (the
 * 16-B-rounded end of the last stream), 1 if payload_cap was too small,
 * streams, moved (the ordering stage's), the sum of skip mod 2^32}.
 * d_payload NULL is RXG_EINVAL; n == 0 or an empty tcb id space zeroes the
 * totals.  The device workspace grows on demand (stream-ordered). */
int rxg_tcp_assemble_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                         const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                         const rxg_verdict *d_v, rxg_segment *d_seg, rxg_tcp_stream *d_stream,
                         uint8_t *d_payload, uint64_t payload_cap, uint32_t *d_totals, void *stream);
/* The same rule on already ordered records in host memory (no device, no
 * context): stream (room for nseg) gets the streams, offset as the device
 * lays them out, *nstream their count; skip / take / dst (room for nseg each)
 * get every record's skipped and taken bytes and the offset of its taken
 * bytes in that layout.  seg is not modified.  nseg == 0 is valid; a NULL
 * argument is RXG_EINVAL.  The CPU path and the tests' second opinion; the
 * device call never falls back to it. */
int rxg_tcp_assemble_host(const rxg_segment *seg, const uint32_t *sip, const uint32_t *avail,
                          uint32_t nseg, rxg_tcp_stream *stream, uint32_t *nstream, uint32_t *skip,
                          uint32_t *take, uint32_t *dst);

/* One mbuf burst through the whole device half of delivery: classify
 * (rxg_process_mbufs), then the UDP compaction (when the UDP id space is at
 * most RXG_COMPACT_MAX_FLOWS; else dgram/first are NULL and ndgram 0) and
 * the TCP segment sort and gather, all in one pass over the staged burst.
 * Verdicts into `out`; the other results stay in pinned buffers the context
 * owns (one set per burst in flight, RXG_DELIVER_DEPTH sets used in turn),
 * valid until the set is reused: RXG_DELIVER_DEPTH delivery calls later.  `ms` (nullable, 8 floats): the
 * phases of this burst in ms — [0] host gather of the mbufs into pinned
 * staging; from HIP events on the device: [1] copy in, [2] classify (K1),
 * [3] the compactions (K3 + K4), [4] copy out of their results; [5] the
 * whole call (host clock); [6], [7] 0.  Synchronous. */
typedef struct rxg_delivery {
    const rxg_dgram *dgram;     /* UDP: as rxg_process_mbufs_udp */
    const uint32_t *first;
    const uint8_t *udp_payload;
    uint32_t ndgram;
    uint32_t nseg;              /* TCP: segments, sorted by (tcb id, frame) */
    uint64_t udp_bytes;
    const rxg_segment *seg;
    const uint8_t *tcp_payload;
    uint64_t tcp_bytes;
    int32_t tcp_payload_ref;    /* >= 0: tcp_payload is pooled buffer `ref`, which the caller
                                   may keep longer with rxg_payload_hold (and must then
                                   rxg_payload_release); -1: valid while the set is (above) */
    uint32_t set;               /* the context's delivery set holding this burst, 1-based
                                   (written by rxg_deliver_submit, read by rxg_deliver_wait) */
} rxg_delivery;
int rxg_process_mbufs_deliver(rxg_ctx *ctx, rxg_mbuf *const *m, uint32_t n, rxg_verdict *out,
                              rxg_delivery *d, float ms[8]);
/* rxg_process_mbufs_deliver in two halves, so the caller can let other work
 * run while the burst is on the GPU: rxg_deliver_submit stages the burst and
 * queues every device step and copy (d gets its buffer pointers), and
 * rxg_deliver_wait(ctx, d, ms) waits for them and fills in d's counts and
 * the phase times.  Up to RXG_DELIVER_DEPTH delivery bursts in flight per
 * context, waited for in any order (a submit while the next set in turn is
 * still in flight is RXG_EINVAL): burst k+1's frames cross PCIe while burst
 * k's results come back and the host delivers burst k-1.  The verdicts of a
 * burst submitted before an earlier one was delivered were classified against
 * the flow tables of that submit.  Between the calls the context's control plane
 * (rxg_flows_add / remove / update / commit-free changes) may run from another
 * thread: rxg_deliver_wait reads none of the flow-table state; any other call
 * on the context waits for rxg_deliver_wait first. */
int rxg_deliver_submit(rxg_ctx *ctx, rxg_mbuf *const *m, uint32_t n, rxg_verdict *out,
                       rxg_delivery *d);
int rxg_deliver_wait(rxg_ctx *ctx, rxg_delivery *d, float ms[8]);

/* Delivery options (0 = the default).  RXG_DLV_TCP_IN_PLACE: the TCP payloads
 * stay where they are, in the caller's frames — the DPDK zero-copy receive,
 * where the socket's fragment points into the mbuf and holds it
 * (rte_mbuf_refcnt_update) until the application has read it, instead of the
 * rte_malloc + rte_memcpy of ng_tcp_enqueue_recvbuffer (tcp.c:133-185).  The
 * device sorts the segments and decodes their records as before but gathers
 * no payload, and only the 32-B records cross PCIe back:
 * rxg_delivery.tcp_payload is NULL and each record's offset is its payload's
 * offset in its frame (34 + 4*hl; ncopy captured bytes).  The caller keeps
 * the frames in place for as long as it points into them. */
#define RXG_DLV_TCP_IN_PLACE 0x1u
/* RXG_DLV_TCP_GRO: the TCP half of a delivery burst runs the coalescing form
 * of K4 (rxg_tcp_coalesce_dev) with the window of rxg_tune_gro (W bytes; 0
 * restores the default, RXG_GRO_DEFAULT_WINDOW): the records' offsets are
 * byte-contiguous inside a run, and the runs cross PCIe with the records
 * (rxg_delivery_runs).  The pooled payload buffers work unchanged.  Not with
 * RXG_DLV_TCP_IN_PLACE (RXG_EINVAL): payloads that stay in their frames
 * cannot be made contiguous.  Off by default. */
#define RXG_DLV_TCP_GRO 0x2u
/* RXG_DLV_TCP_ORDER: the TCP half of a delivery burst runs the ordering form
 * of K4 (rxg_tcp_compact_ordered_dev; the rule: "TCP sequence ordering"):
 * alone, with RXG_DLV_TCP_GRO (W = the window of rxg_tune_gro) or with
 * RXG_DLV_TCP_IN_PLACE (records only).  struct rxg_delivery is unchanged;
 * rxg_delivery_moved reports the burst's count of moved records.  Off by
 * default. */
#define RXG_DLV_TCP_ORDER 0x4u
/* RXG_DLV_TCP_ASSEMBLE: the TCP half of a delivery burst runs the stream
 * assembly (rxg_tcp_assemble_dev; the rule: "TCP stream assembly").  It
 * implies ordering: with RXG_DLV_TCP_ORDER it behaves the same.  Not with
 * RXG_DLV_TCP_GRO or RXG_DLV_TCP_IN_PLACE (RXG_EINVAL): the streams are the
 * coalesced form, and they are gathered.  May be combined with RXG_DLV_DDOS.
 * struct rxg_delivery is unchanged (seg[].ncopy = take, offset into
 * tcp_payload); the streams cross PCIe with the records
 * (rxg_delivery_streams), rxg_delivery_moved keeps working, and the pooled
 * payload buffers work unchanged.  Off by default.  (0x8 is not a flag.) */
#define RXG_DLV_TCP_ASSEMBLE 0x20u
int rxg_tune_deliver(rxg_ctx *ctx, uint32_t flags);
int rxg_tune_gro(rxg_ctx *ctx, uint32_t W);
/* The streams of a waited-for delivery burst: *stream / *nstream, valid as
 * long as the burst's delivery set is; NULL / 0 when RXG_DLV_TCP_ASSEMBLE was
 * off for it. */
int rxg_delivery_streams(rxg_ctx *ctx, const rxg_delivery *d, const rxg_tcp_stream **stream,
                         uint32_t *nstream);
/* The runs of a waited-for delivery burst: *run / *nrun, valid as long as the
 * burst's delivery set is; NULL / 0 when RXG_DLV_TCP_GRO was off for it. */
int rxg_delivery_runs(rxg_ctx *ctx, const rxg_delivery *d, const rxg_tcp_run **run,
                      uint32_t *nrun);
/* The moved count of a waited-for delivery burst; 0 when RXG_DLV_TCP_ORDER
 * was off for it. */
int rxg_delivery_moved(rxg_ctx *ctx, const rxg_delivery *d, uint32_t *moved);

/* Keep a burst's TCP payload buffer (rxg_delivery.tcp_payload_ref) alive past
 * the context's next burst call — e.g. while receive fragments that point into
 * it wait in a socket's ring — and let it go again.  Holds are counted; a
 * buffer is reused once none is left.  RXG_PAYLOAD_BUFS buffers of max_bytes
 * are pinned at most; with all of them held, the payloads of a burst come in
 * the context's own buffer (tcp_payload_ref -1) and must be copied.  Both
 * calls are safe from any thread (atomic counts). */
#define RXG_PAYLOAD_BUFS 6
#define RXG_DELIVER_DEPTH 2
int rxg_payload_hold(rxg_ctx *ctx, int32_t ref);
int rxg_payload_release(rxg_ctx *ctx, int32_t ref);

/* ---- Entropy flood detector (K6, csrc/rx_ddos.hip; opt-in)
 * The reference passes every received frame through an entropy-based flood
 * detector before the burst goes into the protocol ring (ddos_detect,
 * .vscode/test.c:2846-2891, called at :2992-2997).  The rule, restated:
 *   per frame j: set_j = the number of 1-bits in its len bytes, tot_j = 8 * len;
 *   e(s, t) = (-s)*(log2 s - log2 t) - (t-s)*(log2(t-s) - log2 t) + log2 t,
 *   in double, left to right as written (rxg_ddos_entropy);
 *   the state is a ring of RXG_DDOS_WINDOW slots of (set, tot) and the alarm
 *   flag; frame g (counted since the state was fresh) takes slot g mod 256;
 *   frames g < 256 fill their slot and are not checked: the flag is untouched;
 *   from g = 256 on, each frame writes its slot and is checked on the window
 *   g-255 .. g:  S = sum set, T = sum tot (u32), E = sum e (double),
 *   D = E - e(S, T), alarm = (thresh < D), and the flag becomes alarm.
 * e is undefined for s == 0 or s >= t (the reference's NaN: 0 * -inf, the
 * empty frame included).  A window that holds such a frame is undefined: D
 * reads NaN, there is no alarm and the flag becomes 0, as the reference's NaN
 * comparison does; "undefined" is decided from the integers.
 * Divergences from the reference: the length is the frame's len, not the
 * mbuf's buffer size (pkt->buf_len), and bytes past len never count (the
 * reference's count_bit reads whole 8-byte words past the end); an alarm is
 * only reported (the reference calls rte_exit on a rising alarm); thresh is a
 * parameter (1200.0 in the reference).  This is the reference's statistic; no
 * claim is made about its quality as a detector.
 *
 * rxg_ddos_state: zero-filled = fresh; the same layout on host and device. */
#define RXG_DDOS_WINDOW 256u
#define RXG_DDOS_TILE 256u /* frames per block of the device window pass */
#define RXG_DDOS_DEFAULT_THRESH 1200.0
typedef struct rxg_ddos_state {
    uint64_t frames_seen;
    uint32_t flag;  /* the current alarm state, 0 / 1 */
    uint32_t _r0;   /* 0 */
    uint32_t set[RXG_DDOS_WINDOW];
    uint32_t tot[RXG_DDOS_WINDOW];
} rxg_ddos_state;   /* 2064 bytes */
/* per-frame flag bits */
#define RXG_DDOS_WARMUP 0x01u /* g < 256: not checked */
#define RXG_DDOS_UNDEF 0x02u  /* checked, the window is undefined */
#define RXG_DDOS_ALARM 0x04u  /* checked, thresh < D */
#define RXG_DDOS_RISE 0x08u   /* checked, the alarm rose on this frame */
#define RXG_DDOS_FALL 0x10u   /* checked, the alarm fell on this frame */
typedef struct rxg_ddos_summary {
    uint64_t frames_seen;  /* after the burst */
    double last_stat;      /* D of the burst's last frame; NaN: not checked, or undefined */
    uint32_t alarm_frames; /* frames with RXG_DDOS_ALARM */
    uint32_t first_alarm;  /* the first one's index in the burst, or 0xFFFFFFFF */
    uint32_t rises, falls;
    uint32_t undef_frames; /* frames with RXG_DDOS_UNDEF */
    uint32_t flag;         /* the alarm state after the burst */
    uint32_t last_set, last_tot; /* S, T of the burst's last frame (0 when not checked) */
} rxg_ddos_summary;        /* 48 bytes */
/* One burst through the detector on the device, asynchronous on `stream`.
 * Frames as for rxg_classify_dev (d_off << off_unit_log2, off_unit_log2 >= 4).
 * d_state is the caller's device buffer (several detectors can coexist);
 * calls that share a state must be ordered by the caller, and so must calls
 * on one context (they share its workspace, grown on demand in stream order).
 * Per-frame outputs, each nullable: d_bits[j] = set_j, d_flag[j] = the
 * RXG_DDOS_* bits, d_stat[j] = D, or NaN where the frame was not checked or
 * its window is undefined.  d_summary is required and always written.  n == 0
 * is valid and leaves the state as it is.  len_hint (typical frame length,
 * 0 = unknown) picks the lanes per frame of the bits pass unless rxg_tune_ddos
 * forces one.  RXG_EINVAL for a NaN thresh or off_unit_log2 < 4. */
int rxg_ddos_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
                 uint32_t n, uint32_t off_unit_log2, uint32_t len_hint, double thresh,
                 rxg_ddos_state *d_state, uint32_t *d_bits, uint8_t *d_flag, double *d_stat,
                 rxg_ddos_summary *d_summary, void *stream);
/* The two passes of rxg_ddos_dev apart (tools/ddos_sweep.py times them so):
 * the bits pass alone (d_bits required), and the window pass with the state
 * update on bits already computed.  Argument rules as above. */
int rxg_ddos_bits_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                      const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2, uint32_t len_hint,
                      uint32_t *d_bits, void *stream);
int rxg_ddos_window_dev(rxg_ctx *ctx, const uint32_t *d_bits, const uint16_t *d_len, uint32_t n,
                        double thresh, rxg_ddos_state *d_state, uint8_t *d_flag, double *d_stat,
                        rxg_ddos_summary *d_summary, void *stream);
/* The CPU statement of the rule (no device, no context): a literal
 * restatement that sums in slot order like the reference, with libm's log2.
 * The same arguments on host memory; the tests' second opinion, and the
 * detector of the host-verdict path.  The device calls never fall back to it. */
int rxg_ddos_host(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                  uint32_t off_unit_log2, double thresh, rxg_ddos_state *state, uint32_t *bits,
                  uint8_t *flag, double *stat, rxg_ddos_summary *summary);
/* e(s, t) as the reference writes it (ddos_entropy, test.c:2774-2780). */
double rxg_ddos_entropy(double set_bits, double total_bits);
/* Lanes per frame of the bits pass: 1, 8 or 64; 0 = chosen from len_hint.
 * Anything not compiled in is RXG_EINVAL. */
int rxg_tune_ddos(rxg_ctx *ctx, uint32_t lanes_per_frame);
/* RXG_DLV_DDOS (rxg_tune_deliver, combinable with the three flags above): a
 * delivery burst also runs the detector over its staged frames on the
 * context's stream, against the context's own device state, with the
 * threshold of rxg_tune_ddos_thresh (RXG_DDOS_DEFAULT_THRESH until set; NaN
 * is RXG_EINVAL).  The window follows submit order, two bursts in flight
 * included.  Detection only: verdicts, records and payloads are what they are
 * without it, and only the summary crosses PCIe.  rxg_delivery_ddos returns
 * the summary of a waited-for burst (zeroed when the flag was off for it);
 * rxg_ddos_reset makes the context's state fresh.  struct rxg_delivery is
 * unchanged.  Off by default. */
#define RXG_DLV_DDOS 0x10u /* (0x8 is not a flag: rxg_tune_deliver keeps refusing it) */
int rxg_tune_ddos_thresh(rxg_ctx *ctx, double thresh);
int rxg_ddos_reset(rxg_ctx *ctx);
int rxg_delivery_ddos(rxg_ctx *ctx, const rxg_delivery *d, rxg_ddos_summary *summary);

/* ---- SYN cookies (K7, csrc/rx_syncookie.hip; opt-in)
 * A listener answers SYNs and checks handshake ACKs without keeping state: the
 * SYN-ACK's sequence number is a keyed hash of the connection, and the ACK that
 * returns it proves the handshake.  The rule, on frame bytes with this
 * project's conventions (IHL ignored, TCP header at 34, nothing past the
 * captured length is read):
 *   H = SipHash-2-4(k0, k1, M), 64-bit output, M = three little-endian words:
 *     w0 = sip | (u64)dip << 32          (raw loads of frame bytes 26-29, 30-33)
 *     w1 = sport | dport << 16 | (u64)isn << 32   (raw loads of 34-35, 36-37;
 *                                          isn: the client's, host order)
 *     w2 = t                             (the 32-bit time counter)
 *   cookie(tuple, isn, t) = ((t & 0xFF) << 24) | (H & 0xFFFFFF)
 * Frame i is a candidate when len[i] >= 54, its verdict has cls RXG_CLS_TCP
 * and rc RXG_RC_OK, flow_id < id_space and bit flow_id of the listener mask is
 * set.  With fl = byte 47, seq = BE bytes 38-41, ack = BE bytes 42-45:
 *   (fl & 0x17) == 0x02 (SYN; no ACK, RST, FIN): RXG_CK_SYN, and one descriptor:
 *     kind RXG_TXD_TCP, dst_mac = bytes 6-11, src_mac = bytes 0-5, sip / dip and
 *     sport / dport swapped (raw), seq = cookie(tuple, isn = seq, t),
 *     ack = seq + 1, tcp_flags 0x12, hdrlen_off 0x50, optlen 0, window =
 *     p.window, urp = pay_off16 = pay_len = 0;
 *   (fl & 0x16) == 0x10 (ACK; no SYN, RST; FIN and data allowed): with
 *     c = ack - 1, isn = seq - 1, age = ((t & 0xFF) - (c >> 24)) & 0xFF:
 *     RXG_CK_ACK_OK iff age <= max_age and (c & 0xFFFFFF) ==
 *     (H(tuple, isn, t - age) & 0xFFFFFF), t - age mod 2^32; else RXG_CK_ACK_BAD;
 *   anything else, and every non-candidate: 0.
 * Descriptors are compacted in burst order (the k-th SYN's is txd[k]); totals =
 * {SYNs answered, ACK_OK, ACK_BAD, 0}; no descriptor at or past totals[0] and
 * no status byte at or past n is written.  The SYN-ACK carries no options (no
 * MSS is encoded), as every SYN-ACK of the socket layer. */
struct rxg_txd; /* the send descriptor, defined below (TX encode) */
typedef struct rxg_ck_params {
    uint64_t k0, k1;   /* LE64 of key bytes 0-7 and 8-15 */
    uint32_t t;        /* the time counter */
    uint32_t max_age;  /* counters an ACK's cookie may be old, <= 255 */
    uint16_t window;   /* the SYN-ACK's window field, stored as it is */
    uint16_t _r0;
    uint32_t _r1;
} rxg_ck_params;       /* 32 bytes */
#define RXG_CK_SYN 1
#define RXG_CK_ACK_OK 2
#define RXG_CK_ACK_BAD 3
#define RXG_CK_DEFAULT_MAX_AGE 2u
/* cookie(tuple, isn, t); host, pure.  rxg_siphash24 is the hash it uses, on
 * any message (for the published known answers). */
uint32_t rxg_syncookie_value(uint64_t k0, uint64_t k1, uint32_t sip, uint32_t dip, uint16_t sport,
                             uint16_t dport, uint32_t isn, uint32_t t);
uint64_t rxg_siphash24(uint64_t k0, uint64_t k1, const uint8_t *msg, uint64_t len);
/* One burst on the device, asynchronous on `stream`.  Frames as for
 * rxg_classify_dev (off_unit_log2 >= 4, 16-B aligned frame starts), d_v the
 * burst's 16-B verdicts, d_lmask one bit per TCP control block id
 * ((id_space + 31) / 32 words).  *p is read at call time.  d_status: n bytes;
 * d_txd: room for n descriptors, 16-B aligned; d_totals: 4 words, always
 * written.  n == 0 or id_space == 0 zeroes the totals (and the n status bytes)
 * without a launch.  RXG_EINVAL for max_age > 255 and for NULL outputs.  Calls
 * on one context share its workspace (grown on demand in stream order) and
 * must be ordered by the caller. */
int rxg_syncookie_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
                      uint32_t n, uint32_t off_unit_log2, const rxg_verdict *d_v,
                      const uint32_t *d_lmask, uint32_t id_space, const rxg_ck_params *p,
                      uint8_t *d_status, struct rxg_txd *d_txd, uint32_t *d_totals, void *stream);
/* The same on the CPU (csrc/rx_syncookie_host.cpp): no context, no device; the
 * path of callers without a GPU and the tests' second opinion, never a
 * fallback the device call takes. */
int rxg_syncookie_host(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                       uint32_t off_unit_log2, const rxg_verdict *v, const uint32_t *lmask,
                       uint32_t id_space, const rxg_ck_params *p, uint8_t *status, struct rxg_txd *txd,
                       uint32_t totals[4]);
/* RXG_DLV_SYNCOOKIE (rxg_tune_deliver, combinable with every other flag): a
 * delivery burst also runs K7 on the context's stream behind K1, with the
 * parameters and listeners of rxg_syncookie_set (the mask is uploaded in stream
 * order, ahead of the next submit) and the counter of rxg_syncookie_tick.  The
 * n status bytes, an upper-bound copy of n descriptors and the totals cross
 * PCIe with the other results; verdicts, records and payloads are what they
 * are without the flag.  rxg_delivery_cookies returns them for a waited-for
 * burst, valid as long as the burst's delivery set is; NULL / 0 when the flag
 * was off for it.  Without rxg_syncookie_set no frame is a candidate.  struct
 * rxg_delivery is unchanged.  Off by default.  (0x40 is not a flag:
 * rxg_tune_deliver keeps refusing it.) */
#define RXG_DLV_SYNCOOKIE 0x80u
int rxg_syncookie_set(rxg_ctx *ctx, const rxg_ck_params *p, const uint32_t *listener_ids, uint32_t nl);
int rxg_syncookie_tick(rxg_ctx *ctx, uint32_t t);
int rxg_delivery_cookies(rxg_ctx *ctx, const rxg_delivery *d, const uint8_t **status,
                         const struct rxg_txd **txd, uint32_t *ntxd, uint32_t totals[4]);

/* ---- L2 responder (K8, csrc/rx_l2.hip; opt-in)
 * ARP requests for a local address and ICMP echo requests to one are answered
 * on the device: K1 keeps handing both to KNI (cls RXG_CLS_ARP /
 * RXG_CLS_IPV4_OTHER, rc RXG_RC_KNI, on or off), and this pass, behind K1,
 * writes the complete answer frames.  Addresses are raw network order; offsets
 * are frame offsets; nothing past a frame's captured length is read (beyond
 * the 16-B piece that holds its last byte); nlocal == 0 makes no frame a
 * candidate.
 * ARP: frame i is a candidate when its verdict has cls RXG_CLS_ARP,
 *   len >= 42, bytes 14-19 are 00 01 08 00 06 04, the Ethernet source is not a
 *   group address (byte 6 & 1 == 0) and the target protocol address (bytes
 *   38-41) equals some local[j].ip (first match).  Opcode (BE bytes 20-21) 1:
 *   RXG_L2_ARP_REQ, answered; 2: RXG_L2_ARP_REPLY, not answered (the frame is
 *   addressed to us); any other: 0.  The answer (42 bytes, RFC 826 opcode 2):
 *   dst = request bytes 22-27 (sha), src = local[j].mac, type 0806,
 *   00 01 08 00 06 04 00 02, sha = local[j].mac, spa = the request's tpa,
 *   tha = the request's sha, tpa = the request's spa.
 * Echo: frame i is a candidate when its verdict has cls RXG_CLS_IPV4_OTHER,
 *   len >= 42, byte 14 is 0x45 (a header with options is not answered: this
 *   pass does not apply the "IHL ignored" convention), byte 23 is 1,
 *   (BE16(20-21) & 0x3FFF) == 0 (no fragment), byte 6 & 1 == 0, bytes 30-33
 *   equal some local[j].ip, byte 34 is 8, byte 35 is 0, and tl = BE16(16-17)
 *   is >= 28.  M = bytes [34, 14 + tl).  If 14 + tl > len, or the
 *   one's-complement sum of M (odd tail byte padded with zero, stored checksum
 *   included) does not fold to 0xFFFF: RXG_L2_ECHO_BAD, nothing written.
 *   Otherwise RXG_L2_ECHO, answered.  The answer (14 + tl bytes): dst = request
 *   bytes 6-11, src = local[j].mac, type 0800; a fresh IPv4 header as the TX
 *   encoders below write it (45 00, tl, id 0, fragment 0, ttl 64, proto 1,
 *   header checksum the plain complement, sip = request dip, dip = request
 *   sip); ICMP type 0, code 0, then request bytes [38, 14 + tl) unchanged; the
 *   ICMP checksum at 36-37 is computed over the answer's message with its
 *   field taken as 0, plain complement (a sum of 0xFFFF stores 0).
 * Every other frame: status 0.
 * Layout (K5's packed form): answers in burst order, answer k at the
 * 64-B-rounded end of answer k-1 (the first at 0), each zero-filled to its
 * next 64-B boundary; roff[k] in 64-B units, rlen[k] the answer's length,
 * rsrc[k] the index of the frame it answers.  The first answer whose slot
 * would pass cap_bytes ends the output: it and every later answer are not
 * written (status bytes are unaffected).  totals = {ARP_REQ, ARP_REPLY, ECHO,
 * ECHO_BAD frames, answers written, span in 64-B units}.  No byte of the
 * output at or past the span, no roff / rlen / rsrc entry at or past "answers
 * written" and no status byte at or past n is written.  The span of a burst
 * must stay below 2^32 64-B units. */
#define RXG_L2_MAX_LOCAL 8
typedef struct rxg_l2_params {
    uint32_t nlocal; /* <= RXG_L2_MAX_LOCAL */
    struct {
        uint32_t ip;    /* raw network order */
        uint8_t mac[6];
        uint16_t _r;
    } local[RXG_L2_MAX_LOCAL];
} rxg_l2_params; /* 100 bytes */
#define RXG_L2_ARP_REQ 1
#define RXG_L2_ARP_REPLY 2
#define RXG_L2_ECHO 3
#define RXG_L2_ECHO_BAD 4
/* One burst on the device, asynchronous on `stream`.  Frames as for
 * rxg_syncookie_dev (off_unit_log2 >= 4, 16-B aligned frame starts), d_v the
 * burst's 16-B verdicts.  *p is read at call time.  d_status: n bytes (any
 * alignment); d_out: cap_bytes of answer memory, 64-B aligned; d_roff /
 * d_rlen / d_rsrc: room for n entries; d_totals: 6 words, always written.
 * n == 0 zeroes the totals without a launch.  RXG_EINVAL for nlocal >
 * RXG_L2_MAX_LOCAL and for NULL outputs.  Calls on one context share its
 * workspace (grown on demand in stream order) and must be ordered by the
 * caller. */
int rxg_l2_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
               uint32_t n, uint32_t off_unit_log2, const rxg_verdict *d_v, const rxg_l2_params *p,
               uint8_t *d_status, uint8_t *d_out, uint64_t cap_bytes, uint32_t *d_roff,
               uint16_t *d_rlen, uint32_t *d_rsrc, uint32_t *d_totals, void *stream);
/* The same on the CPU (csrc/rx_l2_host.cpp): no context, no device; the path
 * of callers without a GPU and the tests' second opinion, never a fallback the
 * device call takes. */
int rxg_l2_host(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                uint32_t off_unit_log2, const rxg_verdict *v, const rxg_l2_params *p, uint8_t *status,
                uint8_t *out, uint64_t cap_bytes, uint32_t *roff, uint16_t *rlen, uint32_t *rsrc,
                uint32_t totals[6]);
/* RXG_DLV_L2 (rxg_tune_deliver, combinable with every other flag): a delivery
 * burst also runs K8 on the context's stream behind K1, with the parameters
 * and answer capacity of rxg_l2_set (cap_bytes is rounded down to 64 B and
 * bounded by the context's max_bytes + 64 * max_pkts; without rxg_l2_set no
 * frame is a candidate).  The n status bytes, the totals, an upper-bound copy
 * of roff / rlen / rsrc and of the answers' bytes cross PCIe with the other
 * results; verdicts, records and payloads are what they are without the flag.
 * rxg_delivery_l2 returns them for a waited-for burst, valid as long as the
 * burst's delivery set is; NULL / 0 when the flag was off for it.  struct
 * rxg_delivery is unchanged.  Off by default. */
#define RXG_DLV_L2 0x100u
int rxg_l2_set(rxg_ctx *ctx, const rxg_l2_params *p, uint64_t cap_bytes);
int rxg_delivery_l2(rxg_ctx *ctx, const rxg_delivery *d, const uint8_t **status,
                    const uint8_t **frames, const uint32_t **roff, const uint16_t **rlen,
                    const uint32_t **rsrc, uint32_t *nans, uint32_t totals[6]);

/* TX checksum generation (the send side's per-frame work, udp.c:84-95 and
 * tcp.c:444-463): for every IPv4 frame of the burst, the IPv4 header checksum
 * (rte_ipv4_cksum, rte_ip.h:255-265) is written at frame offset 24, and for
 * IPv4 UDP/TCP frames the L4 checksum (rte_ipv4_udptcp_cksum, :325-349; UDP
 * 0 -> 0xFFFF) at offset 40 / 50, each computed with its own field taken as 0
 * and the reference's rx conventions (L4 at ip+20, length tl-20, bytes past
 * the captured length read as 0).  Frames are modified in place; fields not
 * wholly inside the captured length and non-IPv4 frames are left as they are.
 * Device form: asynchronous on `stream`.  Host form: pkts (span_bytes, pinned
 * for speed) is copied to the device, checksummed and copied back; synchronous. */
int rxg_tx_cksum_dev(rxg_ctx *ctx, uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
                     uint32_t n, uint32_t off_unit_log2, uint32_t len_hint, void *stream);
int rxg_tx_cksum(rxg_ctx *ctx, uint8_t *pkts, uint64_t span_bytes, const uint32_t *off,
                 const uint16_t *len, uint32_t n, uint32_t off_unit_log2);

/* TX encode (K5, csrc/tx_encode.hip): complete outgoing frames from send
 * descriptors and payloads, both checksums filled, in one pass.  The frame of
 * a descriptor is byte for byte what the reference's encoders write:
 *   RXG_TXD_UDP  ng_encode_udp_apppkt udp.c:59-98     42 + pay_len bytes
 *   RXG_TXD_TCP  ng_encode_tcp_apppkt tcp.c:420-466   54 + 4*optlen + pay_len
 *   RXG_TXD_ARP  ng_encode_arp_pkt    common.c:206-241 42 (request, opcode 1)
 * IPv4 id and fragment fields 0, ttl 64 (udp.c:74-85, tcp.c:434-445); the
 * IPv4 header checksum (rte_ipv4_cksum: the plain complement, so a sum of
 * 0xFFFF stores 0) at offset 24 and the L4 checksum
 * (rte_ipv4_udptcp_cksum, UDP 0 -> 0xFFFF) at 40 / 50 are those
 * rxg_tx_cksum fills; every frame is zero-filled to its next 64-B boundary.
 * The descriptor is 48 bytes, 16-B aligned (offsets in the comments). */
enum { RXG_TXD_UDP = 0, RXG_TXD_TCP = 1, RXG_TXD_ARP = 2 };
typedef struct rxg_txd {
    uint8_t dst_mac[6];    /* @0  Ethernet destination; ARP: the target-MAC field (all-ones ->
                                  Ethernet destination all-zero, common.c:216-223) */
    uint8_t src_mac[6];    /* @6  (ARP: also the sender MAC) */
    uint32_t sip, dip;     /* @12 @16 raw network order; ARP: sender / target ip */
    uint16_t sport, dport; /* @20 @22 raw */
    uint32_t seq, ack;     /* @24 @28 host order (tcp_fragment.seqnum / acknum; written htonl) */
    uint16_t window, urp;  /* @32 @34 stored as they are (no htons, tcp.c:454) */
    uint8_t hdrlen_off;    /* @36 */
    uint8_t tcp_flags;     /* @37 */
    uint8_t optlen;        /* @38 option words, written as zeros (tcp.c:420-466) */
    uint8_t kind;          /* @39 RXG_TXD_* */
    uint32_t pay_off16;    /* @40 payload start in the payload buffer, 16-B units */
    uint32_t pay_len;      /* @44 payload bytes (UDP/TCP; ARP: ignored) */
} rxg_txd;

/* flags: leave both checksum fields 0 (nstack_tx_burst with cksum == 0) */
#define RXG_TXE_NO_CKSUM 0x1u

/* Device form, asynchronous on `stream`.  d_txd: n descriptors (16-B
 * aligned); d_payload: the payload buffer (16-B aligned; it extends to the
 * next 16-B boundary after every payload, the rule frames follow); d_pkts:
 * cap_bytes of frame memory (64-B aligned).  slot_bytes == 0 packs the
 * frames: frame k follows frame k-1 at 64-B alignment (a layout pass: tile
 * sums, a scan, per-tile offsets, as rxg_gather_dev); slot_bytes != 0 (a
 * multiple of 64) puts frame k at k * slot_bytes.  Outputs: d_off[k] (64-B
 * units, the layout of nstack_tx_burst and rxg_gather_dev), d_len[k], and
 * d_totals = {frames written, span bytes low, span bytes high, frames
 * skipped} (span = end of the last written frame's 64-B slot).  A descriptor
 * is skipped when its kind is unknown, its frame would exceed 65535 bytes or
 * slot_bytes, or its slot would pass cap_bytes; it writes nothing and gets
 * d_off[k] = d_len[k] = 0.  Packed: a descriptor skipped for its kind or
 * length takes no space; the first frame that would pass cap_bytes ends the
 * burst (it and every later descriptor are skipped, as nstack_tx_burst stops
 * at a full buffer).  Bytes outside [slot start, 64-B-rounded frame end) are
 * never written.  len_hint: typical frame length (0 = unknown), chooses the
 * kernel variant only.  d_totals is required (n == 0 zeroes it).  Uses the
 * context's split / gather workspace. */
int rxg_tx_encode_dev(rxg_ctx *ctx, const rxg_txd *d_txd, uint32_t n, const uint8_t *d_payload,
                      uint8_t *d_pkts, uint64_t cap_bytes, uint32_t slot_bytes, uint32_t *d_off,
                      uint16_t *d_len, uint32_t len_hint, uint32_t flags, uint32_t *d_totals,
                      void *stream);
/* Host form (packed): descriptors and payloads (payload_bytes: every payload
 * must end inside it, else RXG_EINVAL) go up, the frames with off / len come
 * back; synchronous.  *span = bytes of pkts used.  RXG_ERANGE if any
 * descriptor was skipped (the others are written). */
int rxg_tx_encode(rxg_ctx *ctx, const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                  uint64_t payload_bytes, uint8_t *pkts, uint64_t cap_bytes, uint32_t *off,
                  uint16_t *len, uint32_t flags, uint64_t *span);
/* The same on the CPU (csrc/tx_encode_host.cpp): no context, no device; the
 * path for callers without a GPU and the tests' reference, never a fallback
 * the device calls take.  slot_bytes as rxg_tx_encode_dev (0 = packed);
 * totals (nullable) as d_totals.  Reads exactly pay_len bytes per payload. */
int rxg_tx_encode_host(const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                       uint64_t payload_bytes, uint8_t *pkts, uint64_t cap_bytes,
                       uint32_t slot_bytes, uint32_t *off, uint16_t *len, uint32_t flags,
                       uint64_t *span, uint32_t totals[4]);

/* TX encode with TCP segmentation (TSO): a RXG_TXD_TCP descriptor whose
 * payload is longer than `mss` becomes s = ceil(pay_len / mss) frames from
 * the one descriptor, the payload read once.  Segment j (0 <= j < s) is the
 * frame ng_encode_tcp_apppkt (tcp.c:420-466) writes for the descriptor with
 * payload bytes [j*mss, min((j+1)*mss, pay_len)), seq + j*mss (mod 2^32), and
 * FIN (0x01) / PSH (0x08) cleared unless j == s-1; everything else (MACs,
 * addresses, ports, ack, window, urp, hdrlen_off, zero option words) is the
 * descriptor's, both checksums are filled per segment and each frame is
 * zero-filled to its 64-B boundary.  UDP and ARP descriptors are never cut by
 * this call (rxg_tx_encode_frag_dev below fragments UDP datagrams); pay_len 0
 * gives one segment.  mss == 0: nothing is
 * cut; mss must be a multiple of 4 (RXG_EINVAL), so that every segment's
 * payload starts 4-B aligned in the payload buffer and lands 2 mod 4 in its
 * frame, the one phase the kernel's funnel knows.
 *
 * Output is per entry (frame), not per descriptor:
 *  1. s_k, the segment count of descriptor k, follows from its kind and
 *     lengths alone: 0 for an unknown kind, or when a segment's frame
 *     (hdr + min(mss, pay_len); the whole frame for UDP / ARP / mss == 0)
 *     exceeds 65535 bytes or slot_bytes.  Descriptor k owns the entries
 *     [first_k, first_k + max(1, s_k)), first_k = sum over i < k of
 *     max(1, s_i) in 64 bits; d_first[k] = first_k, saturated at 2^32-1.
 *  2. A descriptor is written whole or not at all: iff s_k > 0,
 *     first_k + s_k <= out_cap (the capacity of d_off / d_len in entries)
 *     and its frames fit cap_bytes.
 *  3. Packed (slot_bytes == 0): its segments follow each other at 64-B
 *     alignment, and the first descriptor that does not fit cap_bytes ends
 *     the burst.  Slots: entry e sits at e * slot_bytes.
 *  4. A written descriptor gets d_nseg[k] = s_k and off (64-B units) / len
 *     for its entries; a skipped one d_nseg[k] = 0 and off = len = 0 for each
 *     of its entries below out_cap.
 *  5. Bytes outside [slot start, 64-B-rounded frame end) of written frames
 *     are never touched; nothing is written at or past entry out_cap.
 * d_totals has 8 words: {frames written, span bytes low, high, descriptors
 * skipped, entries needed low, high, 0, 0}.  With mss == 0 (or every TCP
 * pay_len <= mss) and out_cap >= n, pkts / off / len / totals[0..3] are those
 * of rxg_tx_encode_dev, first[k] = k and nseg[k] = (len[k] != 0).  The kernel
 * variant is chosen as rxg_tx_encode_dev chooses it (len_hint, rxg_tune_txe).
 * The workspace also holds an entry -> descriptor map of out_cap words and a
 * position word per descriptor. */
int rxg_tx_encode_tso_dev(rxg_ctx *ctx, const rxg_txd *d_txd, uint32_t n, const uint8_t *d_payload,
                          uint32_t mss, uint8_t *d_pkts, uint64_t cap_bytes, uint32_t slot_bytes,
                          uint32_t *d_off, uint16_t *d_len, uint32_t out_cap, uint32_t *d_first,
                          uint32_t *d_nseg, uint32_t len_hint, uint32_t flags, uint32_t *d_totals,
                          void *stream);
/* Host form (packed), as rxg_tx_encode: off / len hold out_cap entries, first
 * / nseg n descriptors.  RXG_ERANGE if any descriptor was skipped; RXG_EINVAL
 * for a bad mss or a payload that ends past payload_bytes. */
int rxg_tx_encode_tso(rxg_ctx *ctx, const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                      uint64_t payload_bytes, uint32_t mss, uint8_t *pkts, uint64_t cap_bytes,
                      uint32_t *off, uint16_t *len, uint32_t out_cap, uint32_t *first,
                      uint32_t *nseg, uint32_t flags, uint64_t *span);
/* The same on the CPU (csrc/tx_encode_host.cpp), as rxg_tx_encode_host;
 * totals (nullable) has 8 words. */
int rxg_tx_encode_tso_host(const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                           uint64_t payload_bytes, uint32_t mss, uint8_t *pkts, uint64_t cap_bytes,
                           uint32_t slot_bytes, uint32_t *off, uint16_t *len, uint32_t out_cap,
                           uint32_t *first, uint32_t *nseg, uint32_t flags, uint64_t *span,
                           uint32_t totals[8]);
/* Sizes the outputs of a burst (host, no device): *entries = the sum of
 * max(1, s_k) (what out_cap must reach for nothing to be skipped for it),
 * *packed_bytes = the packed frames' bytes (slot_bytes == 0) if nothing is
 * skipped for capacity.  Either may be NULL.  RXG_EINVAL for a bad mss. */
int rxg_tx_tso_count(const rxg_txd *txd, uint32_t n, uint32_t mss, uint64_t *entries,
                     uint64_t *packed_bytes);

/* TX encode with both cuts: TCP segmentation as above and IPv4 fragmentation of
 * UDP datagrams, in one call, because a burst of nstack_tx_burst mixes both
 * kinds.  `mss` is rxg_tx_encode_tso_dev's and cuts only RXG_TXD_TCP; `mtu` is
 * the IPv4 MTU and cuts only RXG_TXD_UDP.  mtu == 0: no datagram is cut; else
 * 68 <= mtu <= 65535 (RXG_EINVAL).  ARP descriptors and unknown kinds are the
 * TSO call's.
 *
 * A UDP descriptor with mtu != 0: let L = 8 + pay_len, the datagram (UDP
 * header and payload), and fp = (mtu - 20) & ~7, the datagram bytes per
 * fragment.
 *  - 20 + L <= mtu: not cut.  One entry, byte for byte the frame of
 *    rxg_tx_encode_dev (id 0, fragment field 0) under its skip rules.
 *  - otherwise s = ceil(L / fp) fragments; fragment j carries datagram bytes
 *    [j*fp, min((j+1)*fp, L)), b_j of them, in a frame of 34 + b_j bytes.
 *    s = 0 (skipped: one entry, off = len = 0) when 20 + L > 65535, or when a
 *    fragment's frame, 34 + min(fp, L), exceeds 65535 bytes or slot_bytes.
 * Fragment j: the descriptor's Ethernet header; IPv4 0x45, tos 0, total length
 * 20 + b_j, id = seq & 0xFFFF of the descriptor (big-endian; an uncut
 * descriptor ignores seq), flags / offset = (j*fp/8) | (j < s-1 ? 0x2000 : 0),
 * ttl 64, proto 17, its own header checksum (rte_ipv4_cksum as above: the
 * plain complement), sip, dip; then its datagram bytes.  Bytes 0-7 of the
 * datagram are {sport, dport, be16(L), checksum}, the checksum
 * rte_ipv4_udptcp_cksum over the whole datagram with the pseudo-header
 * (0 -> 0xFFFF): the value rxg_tx_encode_host writes at offset 40 for the
 * same descriptor uncut, wherever that frame exists.  DF is never set.  With
 * RXG_TXE_NO_CKSUM every IPv4 and the UDP checksum field stay 0.  Every frame
 * is zero-filled to its 64-B boundary.
 *
 * Everything else is the TSO call's rules 1-5 with "segment" read as
 * "fragment": entry ownership by max(1, s_k), a descriptor written whole or
 * not at all, packed frames at 64-B alignment with the first descriptor that
 * does not fit cap_bytes ending the burst, nothing written at or past
 * out_cap, bytes outside [slot start, 64-B-rounded frame end) never touched,
 * d_totals of 8 words.  With mtu == 0 every output equals
 * rxg_tx_encode_tso_dev's with the same mss (and so, with mss == 0 too,
 * rxg_tx_encode_dev's).  The payload is read once: each fragment's lane group
 * leaves the sum of its datagram bytes in a workspace word, and a finish
 * kernel on the same stream adds a datagram's words and stores the two
 * checksum bytes into fragment 0.  Receive-side reassembly is not part of
 * this library (K1 ignores the fragment fields, as the reference does); an
 * ordinary IP stack reassembles what this writes. */
int rxg_tx_encode_frag_dev(rxg_ctx *ctx, const rxg_txd *d_txd, uint32_t n, const uint8_t *d_payload,
                           uint32_t mss, uint32_t mtu, uint8_t *d_pkts, uint64_t cap_bytes,
                           uint32_t slot_bytes, uint32_t *d_off, uint16_t *d_len, uint32_t out_cap,
                           uint32_t *d_first, uint32_t *d_nseg, uint32_t len_hint, uint32_t flags,
                           uint32_t *d_totals, void *stream);
/* Host form (packed), as rxg_tx_encode_tso; RXG_EINVAL also for a bad mtu. */
int rxg_tx_encode_frag(rxg_ctx *ctx, const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                       uint64_t payload_bytes, uint32_t mss, uint32_t mtu, uint8_t *pkts,
                       uint64_t cap_bytes, uint32_t *off, uint16_t *len, uint32_t out_cap,
                       uint32_t *first, uint32_t *nseg, uint32_t flags, uint64_t *span);
/* The same on the CPU (csrc/tx_encode_host.cpp), as rxg_tx_encode_tso_host. */
int rxg_tx_encode_frag_host(const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                            uint64_t payload_bytes, uint32_t mss, uint32_t mtu, uint8_t *pkts,
                            uint64_t cap_bytes, uint32_t slot_bytes, uint32_t *off, uint16_t *len,
                            uint32_t out_cap, uint32_t *first, uint32_t *nseg, uint32_t flags,
                            uint64_t *span, uint32_t totals[8]);
/* rxg_tx_tso_count with both cuts.  RXG_EINVAL for a bad mss or mtu. */
int rxg_tx_frag_count(const rxg_txd *txd, uint32_t n, uint32_t mss, uint32_t mtu, uint64_t *entries,
                      uint64_t *packed_bytes);

/* Tuning hook for the TX encode kernel: force entry `variant` of its variant
 * table (csrc/tx_encode.hip k_txe; RXG_TX_AUTO = chosen from len_hint) and cap
 * its resident blocks per CU (0 = the variant's default). */
int rxg_tune_txe(rxg_ctx *ctx, uint32_t variant, uint32_t blocks_per_cu);

/* Tuning hook: force the kernel variant (lanes per frame 1 or 4..64, passes
 * loaded up front, frames per lane group, pipeline mode; 0xFFFFFFFF = the
 * default pipeline); lanes_per_frame = 0 with pipeline 0xFFFFFFFF =
 * automatic from len_hint; lanes_per_frame = 0 with any other pipeline =
 * that frame-size-independent variant (20: size-class binned path; 30 and
 * up: stream and SH kernel variants; csrc/rx_classify.hip k_variants).  A
 * combination that is not compiled in returns RXG_EINVAL.  Every variant of
 * the product library gives the same verdicts; diagnostic ablations (wrong
 * verdicts by construction) exist only in the RX_DIAG tuning build
 * (librxgpu_diag.so), never in librxgpu.so. */
int rxg_tune(rxg_ctx *ctx, uint32_t lanes_per_frame, uint32_t passes, uint32_t frames_per_group,
             uint32_t pipeline);

/* The classify variant a burst with this len_hint runs on this context (the
 * rxg_tune override, else the default for len_hint): variant = {lanes per
 * frame, passes, frames per group, pipeline}; name (nullable, name_cap bytes
 * with the NUL) = the kernel it dispatches as a kernel trace names it
 * (rocprofv3), without template arguments.  Diagnostics: it lets a benchmark
 * line name the dispatch a profiler shows. */
int rxg_kernel_variant(const rxg_ctx *ctx, uint32_t len_hint, uint32_t variant[4], char *name,
                       uint32_t name_cap);

/* Tuning hook: cap the resident 256-thread blocks per CU the launch uses
 * (0 = as many as the occupancy allows). */
int rxg_tune_grid(rxg_ctx *ctx, uint32_t blocks_per_cu);

/* Tuning hook for the TX checksum kernel: force entry `variant` of its
 * variant table (csrc/tx_cksum.hip k_tx; RXG_TX_AUTO = chosen from len_hint)
 * and cap its resident blocks per CU (0 = the variant's default). */
#define RXG_TX_AUTO 0xFFFFFFFFu
int rxg_tune_tx(rxg_ctx *ctx, uint32_t variant, uint32_t blocks_per_cu);

/* Tuning hook for the exact-key flow tables: load factor <= 2^-load_log2
 * (1 = 1/2, 2 = 1/4, up to 4; 0 = the default), applied by the next
 * rxg_flows_sync.  Verdicts do not depend on it; the table's cache footprint
 * and probe length do. */
int rxg_tune_flow_load(rxg_ctx *ctx, uint32_t load_log2);

/* Tuning hook: flow-table layout flags (0 = the default layout).
 * RXG_TT_NO_UDP_PORT (applied by the next rxg_flows_sync): no direct UDP port
 * table; every UDP lookup probes the hashed table.  RXG_TT_COUNT_4B (applied
 * at once): the 8193..2M-flow count path keeps 4-B count indices even at
 * <= 65536 flows.  RXG_TT_COUNT_2BUF (applied at once): see below.  Verdicts
 * and counts depend on none of them. */
#define RXG_TT_NO_UDP_PORT 0x1u
#define RXG_TT_COUNT_4B 0x2u
#define RXG_TT_COUNT_2BUF 0x4u /* rxg_classify_dev_cs: two count-index buffers instead of
                                  three (each burst then waits for the count of the
                                  burst before the previous one) */
#define RXG_TT_SLAB_HALF 0x8u     /* the count's slab pass on half / a quarter of the CUs */
#define RXG_TT_SLAB_QUARTER 0x10u /* (fewer, larger slabs; applied at once) */

int rxg_tune_tables(rxg_ctx *ctx, uint32_t flags);

/* Tuning hook: how mbuf bursts whose frames lie in registered memory
 * (rxg_register_host) reach the GPU.  RXG_INGEST_AUTO (the default): a burst
 * dense in one region (its covering span at most 1.4x its frames' bytes and
 * within the staging slot) is copied as that one span by the copy engine,
 * any other registered burst is pulled by the device frame by frame;
 * RXG_INGEST_PULL: always pulled; RXG_INGEST_GATHER: always gathered on the
 * host.  Outputs do not depend on it.  In both registered forms the frames
 * are read after the call returns: they must stay in place until the burst
 * is waited for (rxg_deliver_wait; the synchronous calls return after it). */
#define RXG_INGEST_AUTO 0u
#define RXG_INGEST_PULL 1u
#define RXG_INGEST_GATHER 2u
int rxg_tune_ingest(rxg_ctx *ctx, uint32_t mode);

/* Context-owned per-flow counts (accumulated by rxg_classify / rxg_process_mbufs). */
int rxg_flow_counts(rxg_ctx *ctx, uint64_t *counts, uint32_t ncounts);
int rxg_counts_reset(rxg_ctx *ctx);
uint32_t rxg_num_flows(const rxg_ctx *ctx);

/* Diagnostics: flow table `which` (0 UDP slots, 1 TCP slots, 2 listeners,
 * 3 the lane kernel's compact UDP table (8-B slots {dip, dport | flow << 16}),
 * 4 its UDP port window (u16 flow ids, 0xFFFF none)) as the device holds it
 * (device_copy != 0; after this context's bursts drain) or as the host image
 * is, up to `bytes`; info (nullable) = {device tcp_mask, tcp_probe, hseed,
 * host tcp mask, probe, seed, changes pending, slots} for 0-2, and for 3-4
 * {slots - 1 of the compact table, its longest probe, hseed, compact keys off
 * the window's address, window's first port (host order), window length,
 * window's address (raw), entries of `which`}. */
int rxg_ft_dump(rxg_ctx *ctx, uint32_t which, int device_copy, void *dst, uint64_t bytes,
                uint32_t info[8]);

/* Host-side lookups through the built flow table (same code path as the
 * device probe, for control-plane use and tests). */
uint32_t rxg_ft_lookup_udp(const rxg_ctx *ctx, uint32_t dip, uint16_t dport);
uint32_t rxg_ft_lookup_tcp(const rxg_ctx *ctx, uint32_t sip, uint32_t dip, uint16_t sport,
                           uint16_t dport);

/* RSS: Toeplitz hash (standard 40-byte key) over sip,dip,sport,dport in
 * network byte order, as a multi-queue NIC computes it; shard = hash % n. */
uint32_t rxg_rss_hash(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport);

/* ---- multi-GPU: RSS split, shard gather, per-flow count all-reduce ------
 * The reference runs one rx queue (ng_init_port, netfamily.c:38-39) and one
 * pkt_process lcore (netfamily.c:427) over the burst it dequeues at
 * netfamily.c:147.  Across G GPUs of a node the burst is split by RSS, as the
 * multi-queue NIC the README assumes (README.md:13) would: each GPU holds a
 * replica of the flow tables (rxg_flows_sync with the same lists) and
 * classifies its shard; the per-flow counts are the only exchange. */
#define RXG_MAX_SHARDS 64

/* Shard of a frame = rxg_rss_hash(sip, dip, sport, dport) % n_shards for IPv4
 * TCP/UDP, rxg_rss_hash(sip, dip, 0, 0) % n_shards for other IPv4, 0 for
 * non-IPv4 frames (bytes past the captured length read as 0).  perm[] gets
 * the frame indices grouped by shard, in burst order inside a shard;
 * first[s] = start of shard s in perm, first[n_shards] = n (n_shards + 1
 * entries).  Host form: host buffers, synchronous.  Device form: device
 * buffers, asynchronous on `stream` (workspace grown on demand, between
 * bursts).  Readable extent, rxg_rss_split_dev and rxg_gather_dev: each frame
 * must be readable to its 16-B end (pkts + (off << off_unit_log2) rounded up
 * from len to a multiple of 16), and a zero-length frame's offset must be
 * readable for 16 B (the kernels load whole 16-B chunks and mask them). */
int rxg_rss_split(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                  uint32_t off_unit_log2, uint32_t n_shards, uint32_t *first, uint32_t *perm);
int rxg_rss_split_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                      const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2, uint32_t n_shards,
                      uint32_t *d_first, uint32_t *d_perm, void *stream);

/* Gather frames d_idx[0..count) of a device burst into a packed device burst
 * (the DMA of one RSS queue's frames into its ring): frame k at
 * d_dst + (d_dst_off[k] << 6), 64-B aligned, zero-filled to its 64-B end,
 * d_dst_len[k] = its captured length (so the result is classified with
 * off_unit_log2 = 6).  *span = bytes the packed burst occupies.  Synchronises
 * `stream` (setup-time operation); RXG_ERANGE if the packed burst exceeds
 * dst_cap (frames past dst_cap are not copied). */
int rxg_gather_dev(rxg_ctx *ctx, const uint8_t *d_pkts, const uint32_t *d_off,
                   const uint16_t *d_len, uint32_t off_unit_log2, const uint32_t *d_idx,
                   uint32_t count, uint8_t *d_dst, uint64_t dst_cap, uint32_t *d_dst_off,
                   uint16_t *d_dst_len, uint64_t *span, void *stream);

/* A communicator over the GPUs of the node (RCCL over xGMI), one rank per
 * GPU/process.  Rank 0 makes the id with rxg_group_id and the caller hands it
 * to every rank by its own means (a file, a socket, MPI, torch.distributed);
 * every rank then calls rxg_group_open with it (collective: returns once all
 * nranks have joined). */
#define RXG_GROUP_ID_BYTES 128
typedef struct rxg_group rxg_group;
int rxg_group_id(uint8_t id[RXG_GROUP_ID_BYTES]);
int rxg_group_open(rxg_group **g, int device, uint32_t nranks, uint32_t rank,
                   const uint8_t id[RXG_GROUP_ID_BYTES]);
void rxg_group_close(rxg_group *g);
/* The communicator's size and this process's rank as RCCL reports them
 * (ncclCommCount / ncclCommUserRank); either pointer may be NULL. */
int rxg_group_size(const rxg_group *g, uint32_t *nranks, uint32_t *rank);
/* Sum of a device u64 count vector over the ranks, in place, asynchronous on
 * `stream` (every rank must call it with the same n). */
int rxg_counts_allreduce(rxg_group *g, uint64_t *d_counts, uint32_t n, void *stream);
/* The same for the context-owned counts (rxg_classify / rxg_process_mbufs),
 * after every burst submitted so far; synchronous.  Only the increment since
 * the previous call is reduced and then added to the running total, so the
 * context's counts (rxg_flow_counts) are the global totals after each call,
 * however often it is called. */
int rxg_ctx_counts_allreduce(rxg_ctx *ctx, rxg_group *g);

/* ---- pcap ingest (the NIC stand-in: rte_eth_rx_burst into the in-ring,
 * netfamily.c:438-440) -------------------------------------------------- */
/* Classic libpcap files, LINKTYPE_ETHERNET, either byte order, us or ns
 * stamps.  A file is mapped once and read burst by burst in capture order. */
typedef struct rxg_pcap rxg_pcap;
int rxg_pcap_open(rxg_pcap **p, const char *path);
void rxg_pcap_close(rxg_pcap *p);
int rxg_pcap_rewind(rxg_pcap *p);
/* Pack up to max_frames next frames into pkts (cap_bytes) in the burst layout:
 * frame k at off[k] << off_unit_log2, captured length len[k], zero fill to the
 * next 16-B boundary.  *n = frames packed (0 at end of file), *span = bytes
 * used.  A record longer than 65535 bytes is RXG_ERANGE; a truncated file is
 * RXG_EINVAL. */
int rxg_pcap_read_burst(rxg_pcap *p, uint8_t *pkts, uint64_t cap_bytes, uint32_t *off,
                        uint16_t *len, uint32_t max_frames, uint32_t off_unit_log2, uint32_t *n,
                        uint64_t *span);
/* Write n frames of a burst as a pcap file (capture order = burst order). */
int rxg_pcap_write(const char *path, const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                   uint32_t n, uint32_t off_unit_log2);

/* ---- synthetic traffic (pktgen) --------------------------------------- */
/* Deterministic counter-based generator: frame i is a pure function of
 * (cfg, i), identical on host and device.  Frames are written at
 * off[i] = i * (slot_bytes >> off_unit_log2), or packed (cfg.packed). */
typedef struct rxg_gen_cfg {
    uint64_t seed;
    uint32_t size_mode;     /* 0 fixed frame_len, 1 IMIX 64/576/1500 at 7:4:1 */
    uint32_t frame_len;     /* fixed-size frames (>= 64 for TCP/UDP) */
    uint32_t slot_bytes;    /* bytes reserved per frame (multiple of 16, >= max frame) */
    uint32_t proto_mode;    /* 0 UDP only, 1 TCP only, 2 TCP/UDP 50/50 */
    uint32_t n_udp;         /* UDP sockets: local_ip:(udp_base_port + k) */
    uint32_t n_tcp;         /* established tcbs: (10.128.x.y : 1024+..) -> local_ip:tcp_port */
    uint32_t local_ip;      /* network order (192.168.100.77 = netfamily.c:11) */
    uint16_t udp_base_port; /* host order */
    uint16_t tcp_port;      /* host order (9999 = netfamily.c:270) */
    uint32_t bad_cksum_per10k; /* one flipped payload bit after the checksum */
    uint32_t unknown_per10k;   /* destination port with no socket / listener */
    uint32_t other_per10k;     /* ICMP or ARP frames */
    uint32_t shard;         /* keep only tuples whose rxg_rss_hash % n_shards == shard */
    uint32_t n_shards;      /* 1 = no sharding */
    uint32_t packed;        /* 0: frame i in slot i (slot_bytes apart); 1: frames packed
                               back to back at 64-B alignment (what rxg_process_mbufs
                               staging produces); slot_bytes then bounds one frame */
    uint32_t src_ip;        /* network order; != 0: every UDP frame to a bound socket
                               comes from src_ip:src_port (one 5-tuple, e.g. the echo
                               client of BASELINE configs[0]); 0: random sources */
    uint16_t src_port;      /* host order */
    uint16_t _pad;
} rxg_gen_cfg;

/* Flow set the generator assumes (the sockets/tcbs a test or bench binds). */
int rxg_gen_flows(const rxg_gen_cfg *cfg, rxg_udp_sock *u, rxg_tcb *t);
/* Host generation of frames [first, first+n) into caller buffers (slot i-first;
 * the buffer must hold n * slot_bytes bytes in either layout). */
int rxg_gen_host(const rxg_gen_cfg *cfg, uint64_t first, uint32_t n, uint8_t *pkts,
                 uint32_t *off, uint16_t *len, uint32_t off_unit_log2);
/* Device generation (same frames), asynchronous on stream. */
int rxg_gen_dev(const rxg_gen_cfg *cfg, uint64_t first, uint32_t n, uint8_t *d_pkts,
                uint32_t *d_off, uint16_t *d_len, uint32_t off_unit_log2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RXGPU_H */
