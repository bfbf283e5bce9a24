/*
 * nstack.h — socket-style API of the stack, host C, over librxgpu.
 *
 * Same names, signatures and return conventions as the reference's socket
 * layer (common.h:189-200, bodies common.c:262-666), so an application
 * written against the reference (netfamily.c:211-383) links unchanged.  The
 * control blocks are the reference's (struct localhost udp.h:10-29, struct
 * tcp_stream tcp.h:29-55) in the same head-inserted lists; what changes is
 * the receive path: instead of per-frame udp_process/tcp_process calls on the
 * protocol lcore, a burst goes through nstack_rx_burst(), which classifies it
 * on the GPU (rxg_process_mbufs) and then delivers UDP payloads into the
 * sockets' receive rings with the reference's `struct offload` semantics
 * (udp.c:25-52), where nrecvfrom() picks them up.
 *
 * Deliberate differences (DESIGN.md §Socket layer):
 *   - the lists are guarded by a lock (the reference mutates them from the
 *     app lcore while the protocol lcore walks them, common.c:302,336,620,660);
 *   - control blocks are reference-counted: a call blocked in nrecv /
 *     nrecvfrom / naccept on a block that another thread closes (or whose
 *     last ACK frees it) wakes and returns -1 (errno EBADF) instead of
 *     waiting on freed memory;
 *   - get_hostinfo_fromfd walks the list correctly (common.c:116 advances
 *     from the list head and never terminates past the second socket);
 *   - nrecvfrom/nrecv/naccept honour MSG_DONTWAIT in `flags` (the reference
 *     ignores flags and always blocks); naccept has no flags: it blocks;
 *   - the 8 bytes nrecvfrom returns past the payload (offload.length =
 *     dgram_len, udp.c:37, but only dgram_len-8 bytes are stored, udp.c:38) read
 *     as zeros instead of adjacent heap memory.
 * TCP segments that pass classify drive the reference's state machine
 * (tcp.c:43-331, dispatch :373-415) on the host, frame by frame in burst
 * order: LISTEN+SYN creates a tcb and queues SYN|ACK, SYN_RCVD+ACK
 * establishes and wakes naccept, ESTABLISHED+PSH queues the payload for
 * nrecv and an ACK, +FIN queues the EOF marker and moves to CLOSE_WAIT,
 * LAST_ACK+ACK frees the tcb.  A burst is classified against one snapshot of
 * the tcb list; once the burst's own segments change that list (SYN, final
 * ACK), later segments of the burst are looked up again on the live list
 * (through the host image of the flow tables, O(1) per lookup), so the
 * outcome is the reference's sequential one (a SYN and its ACK may share a
 * burst).  Segments of a tcb in ESTABLISHED (or a state whose segments are
 * no-ops) depend on no other frame of the burst: the GPU sorts them per
 * connection and gathers their payloads (rxg_process_mbufs_deliver), and
 * they run connection by connection, each connection's fragments and ACKs
 * queued as one batch (one allocation); every other frame keeps the
 * frame-by-frame path.  Unresolved merge-conflict hunks of tcp.c take the
 * HEAD side.
 */
#ifndef NSTACK_H
#define NSTACK_H

#include <stdint.h>
#include <sys/socket.h>
#include <sys/types.h>

#include "rxgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Process-wide stack, like the reference's globals (netfamily.c:16-18).
 * device = HIP ordinal, or RXG_HOST_ONLY for a stack without a GPU (socket
 * API + nstack_deliver work; nstack_rx_burst returns RXG_ENODEV). */
int nstack_init(int device, uint32_t max_burst, uint64_t max_bytes);
void nstack_fini(void);

/* socket API (common.h:189-200) */
int nsocket(int domain, int type, int protocol);
int nbind(int sockfd, const struct sockaddr *addr, socklen_t addrlen);
int nlisten(int sockfd, int backlog);
int naccept(int sockfd, struct sockaddr *addr, socklen_t *addrlen);
ssize_t nsend(int sockfd, const void *buf, size_t len, int flags);
ssize_t nrecv(int sockfd, void *buf, size_t len, int flags);
ssize_t nrecvfrom(int sockfd, void *buf, size_t len, int flags, struct sockaddr *src_addr,
                  socklen_t *addrlen);
ssize_t nsendto(int sockfd, const void *buf, size_t len, int flags, const struct sockaddr *dest_addr,
                socklen_t addrlen);
int nclose(int fd);

/* Receive burst: the loop body of pkt_process (netfamily.c:152-200) for n
 * frames at once (as two halves in flight together, see nstack_set_halves;
 * the outcome is the same).  rc_out[i] (nullable) = what udp_process/tcp_process would
 * have returned (KNI frames: 1); v_out (nullable) = the verdicts.
 * Returns the number of UDP datagrams delivered, or a negative RXG_E* code.
 * A burst run as two halves whose second half could not go through the GPU
 * after the first was delivered returns, when rc_out is given, the first
 * half's count: the second half's rc_out entries hold the (negative RXG_E*)
 * error and its v_out entries are zero, so the caller can pass those frames
 * again.  With rc_out NULL it returns the error code.
 * Called by one protocol thread, which also runs nstack_tx_burst (as
 * pkt_process runs udp_out / tcp_out); while the burst is on the GPU the
 * stack's lock is released, so application threads' socket calls run beside
 * it (a second concurrent nstack_rx_burst gets RXG_EINVAL). */
int nstack_rx_burst(rxg_mbuf *const *m, uint32_t n, int *rc_out, rxg_verdict *v_out);

/* Pipelined receive: the same delivery as nstack_rx_burst, with the next
 * burst on the GPU (copy in, K1/K3/K4, copy out) while the protocol thread
 * delivers the previous one.  nstack_rx_submit queues a burst and returns at
 * once (RXG_DELIVER_DEPTH = 2 bursts submitted and not completed at most;
 * RXG_EINVAL past that, or while an nstack_rx_burst runs); nstack_rx_complete
 * waits for the oldest submitted burst and delivers it, frame order and
 * outcomes as nstack_rx_burst's, and returns its UDP datagrams delivered (or
 * a negative RXG_E* code: the burst was not delivered, RXG_EINVAL when none
 * is pending).  A burst's frames, rc_out and v_out must stay valid until its
 * complete.  A burst classified before the previous one was delivered is
 * delivered frame by frame on the live lists when that delivery or a socket
 * call changed a lookup (the reference's sequential outcome, netfamily.c:
 * 147-200 taking burst k+1 only after burst k).  The loop:
 *     nstack_rx_submit(b0); for (k...) { nstack_rx_submit(b[k+1]); nstack_rx_complete(); }
 * nstack_rx_pending: bursts submitted and not completed.  nstack_rx_burst and
 * nstack_deliver are refused while any is pending; nstack_fini waits for them
 * and drops them. */
int nstack_rx_submit(rxg_mbuf *const *m, uint32_t n, int *rc_out, rxg_verdict *v_out);
int nstack_rx_complete(void);
int nstack_rx_pending(void);

/* Delivery half only: apply verdicts computed by rxg_* to the frames (UDP ->
 * socket receive rings, TCP -> state machine).  Verdict flow ids are the
 * blocks' stable ids (nstack_flow_ids).  `gen` = the generation nstack_flows
 * returned with the lists the verdicts were classified against: if the lists
 * changed since (a block created, rebound, made a listener or freed — a freed
 * id may be reused), every frame of the burst is looked up again on the live
 * lists, as the reference's per-frame lookups would, instead of trusting the
 * flow ids.  rc_out (nullable) as for nstack_rx_burst. */
int nstack_deliver(rxg_mbuf *const *m, uint32_t n, const rxg_verdict *v, uint64_t gen,
                   int *rc_out);

/* Install a tcb as tcp_stream_create + LL_ADD do on a SYN (tcp.c:3-52) and
 * wake a blocked naccept (tcp.c:108-116).  All values raw network order. */
int nstack_tcb_add(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport, int status);

/* The control blocks in creation order (the lists rxg_flows_sync would
 * take) and the generation of the lists (nullable; for nstack_deliver).
 * Counts are always written; arrays up to their capacities.  Every block is
 * registered with the context's GPU flow tables as it is created, bound,
 * made a listener and freed (nsocket / nbind / nlisten / SYN / last ACK /
 * nclose: rxg_flows_add / update / remove, committed with the next burst), so
 * no burst ever waits for a table rebuild. */
int nstack_flows(rxg_udp_sock *u, uint32_t cap_u, uint32_t *nu, rxg_tcb *t, uint32_t cap_t,
                 uint32_t *nt, uint64_t *gen);
/* The stable flow id (verdict flow_id, count index) of each block of the
 * nstack_flows arrays, in the same order. */
int nstack_flow_ids(uint32_t *uid, uint32_t cap_u, uint32_t *tid, uint32_t cap_t);

/* Diagnostics (tests): the flow id the library's flow tables (the host image
 * of what the device probes) give a key — UDP (dst ip, dst port), TCP (the
 * exact 4-tuple, else the listener on dport); RXG_FLOW_NONE if none. */
uint32_t nstack_lookup_udp(uint32_t dip, uint16_t dport);
/* The mbuf pool's memory (rxg_register_host on the stack's context): bursts
 * whose frames lie in it are pulled by the GPU instead of gathered on the
 * host (DPDK: once per memory chunk of the pool, rte_mempool_mem_iter). */
int nstack_register_host(void *base, uint64_t bytes);
/* the library context the socket layer classifies with (diagnostics) */
rxg_ctx *nstack_ctx(void);
uint32_t nstack_lookup_tcp(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport);

/* Diagnostics (tests): the tcb with this exact 4-tuple (raw network order):
 * status, rcv_nxt, snd_nxt, fd; and the k-th fragment queued in its send
 * ring (TCP flags, acknum).  0 = found, -1 = none.  nstack_tcb_count = tcbs
 * in the list (listeners included). */
int nstack_tcb_state(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport, int32_t *status,
                     uint32_t *rcv_nxt, uint32_t *snd_nxt, int32_t *fd);
int nstack_tcb_sndq(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport, uint32_t k,
                    uint8_t *flags, uint32_t *acknum);
uint32_t nstack_tcb_count(void);

/* ---- TX (the udp_out / tcp_out pass of the protocol loop, netfamily.c:205-206)
 * Local identity: gLocalIp (netfamily.c:11) and the port MAC g_stCpuMac
 * (netfamily.c:415).  Frames leave from this MAC (copied into sockets at
 * nbind and into tcbs at creation, as common.c:356,365 / tcp.c:32 do); an
 * ARP frame addressed to this IP teaches the ARP table.  Raw network-order ip. */
int nstack_set_local(uint32_t ip, const uint8_t mac[6]);
/* ng_arp_entry_insert (common.c:177-204): 1 = inserted, 0 = already known */
int nstack_arp_insert(uint32_t ip, const uint8_t mac[6]);
/* One udp_out + tcp_out pass (udp.c:123-164, tcp.c:492-555): at most one
 * queued datagram per UDP socket and one fragment per tcb, in list order,
 * encoded as frames (ng_encode_udp_apppkt udp.c:59-98, ng_encode_tcp_apppkt
 * tcp.c:420-466) into pkts/off/len (the rx burst layout, off in 64-B units).
 * A destination with no ARP entry gets an ARP request (ng_send_arp,
 * common.c:206-260) and its item is queued again, as the reference does.
 * cksum != 0: both checksums are filled on the GPU (rxg_tx_cksum) before the
 * call returns; 0: both fields are left 0.  Items that do not fit stay queued.
 * Returns the number of frames (or a negative RXG_E* code); *span = bytes used. */
int nstack_tx_burst(uint8_t *pkts, uint64_t cap_bytes, uint32_t *off, uint16_t *len,
                    uint32_t max_frames, int cksum, uint64_t *span);
/* on != 0: nstack_tx_burst with cksum != 0 builds its frames on the GPU (K5,
 * rxg_tx_encode).  The two list walks collect send descriptors (rxg_txd; ARP
 * requests included) in the same order and with the same requeue, drop and
 * capacity rules, the payloads go into pinned staging at 16-B aligned
 * offsets, and one rxg_tx_encode call produces the burst: frames, off, len,
 * *span, return value and queue state are those of the host-framed path.
 * Default off; with cksum == 0 the host frames as before.  nstack_stat(13)
 * counts the frames the encoder produced.  Returns 0. */
int nstack_set_tx_encode(int on);
/* TCP segmentation for tcp_out's walk.  mss == 0 (the default): off, a
 * fragment is one frame of any length, as nsend queued it (common.c:418-460).
 * mss != 0 (a multiple of 4, else RXG_EINVAL; rxg_tx_encode_tso's rule): a
 * fragment longer than mss is sent as s = ceil(length / mss) frames with
 * consecutive sequence numbers, FIN / PSH only on the last.  It needs s of
 * max_frames and the segments' 64-B-rounded bytes of cap_bytes.  If only
 * r < s whole segments fit and r > 0, those r go out now with FIN / PSH
 * cleared, the fragment stays at the head of the send queue with seqnum,
 * data and length advanced by r * mss, and the pass is full; r == 0: it
 * stays queued and the pass ends, as at a full buffer.  Both framing paths
 * honour it: the host emits the segments itself, the encoder path
 * (nstack_set_tx_encode) passes one descriptor per fragment to
 * rxg_tx_encode_tso; frames, off, len, *span, return value (frames) and
 * queue state are the same.  The 65535-B drop rule then applies to a
 * segment's frame.  nstack_stat(14) counts the times a fragment went out as
 * more than one frame in a pass.  Returns 0. */
int nstack_set_tx_mss(uint32_t mss);
/* IPv4 fragmentation for udp_out's walk.  mtu == 0 (the default): off, a
 * datagram is one frame of any length up to 65535 bytes.  mtu != 0 (the IPv4
 * MTU, 68..65535, else RXG_EINVAL; rxg_tx_encode_frag's rule): a datagram
 * with an ARP entry and 28 + length > mtu goes out as its s fragments
 * (include/rxgpu.h), all of them or none: it needs s of max_frames and its
 * fragments' 64-B-rounded bytes of cap_bytes.  If it does not fit what is
 * left of the pass it stays queued and the pass is full; if it cannot fit
 * even an empty pass of the caller's size (s > max_frames, or its bytes
 * exceed cap_bytes) it is dropped and counter 1 counts it, so that it cannot
 * block its socket for ever.  The 42 + length > 65535 drop applies only to
 * datagrams that are not cut; the ARP-miss path is unchanged.  The IPv4 id
 * comes from a per-stack 16-bit counter that starts at 1 after init or fini
 * and is bumped once per cut datagram, when it is dequeued.  Both framing
 * paths honour it: the host emits the fragments itself (cksum == 0 leaves
 * the checksum fields 0), the encoder path (nstack_set_tx_encode) passes one
 * descriptor per datagram, the id in its seq, to rxg_tx_encode_frag together
 * with the MSS; frames, off, len, *span, return value and queue state are the
 * same.  DF is never set, there is no path-MTU discovery, and received
 * fragments are not reassembled.  nstack_stat(25) counts the datagrams sent as
 * more than one frame.  nstack_fini resets it.  Returns 0. */
int nstack_set_tx_mtu(uint32_t mtu);

/* The application side of a benchmark, in one call: every UDP socket read
 * with nrecvfrom until empty, every tcb's receive queue read (nrecv) and its
 * queued ACKs taken off its send ring (as one tcp_out pass would).  buf/cap =
 * the receive buffer each call uses.  Returns the datagrams + fragments
 * received (EOF fragments are read and not counted, as oracle_drain_all does;
 * a negative RXG_E* code on error); *bytes = the bytes the calls returned.
 * Never takes the stack's lock: a short lock of the id maps is held to take
 * a reference on the next 8192 blocks; the reads run under each block's own
 * mutex, so a concurrent nstack_rx_burst delivers beside them, and a block
 * freed meanwhile (last ACK) stays valid until the call lets go of it.
 * nrecv / nrecvfrom / nsendto look their descriptor up the same way. */
int64_t nstack_drain_all(void *buf, size_t cap, uint64_t *bytes);
/* nstack_drain_all, and *sum = the sum (mod 2^64) over every datagram and
 * fragment read of the FNV-1a 64 hash of the bytes the read returned: an
 * order-free check of the content the application received (tests). */
int64_t nstack_drain_all_sum(void *buf, size_t cap, uint64_t *bytes, uint64_t *sum);

/* In-place TCP receive (DPDK zero-copy; off by default).  on != 0: a
 * receive fragment whose payload was captured whole is not copied (the
 * rte_malloc + rte_memcpy of ng_tcp_enqueue_recvbuffer, tcp.c:133-185): it
 * points into its frame, and the stack takes a reference on the frame's mbuf
 * (rxg_mbuf.refcnt += 1, atomically, as rte_mbuf_refcnt_update) until the
 * application has read it.  The GPU then sends back only the segment
 * records, no payload (RXG_DLV_TCP_IN_PLACE).  The put that drops an mbuf's
 * count to 0 calls release(m, arg) (nullable; e.g. the mempool's free, as
 * rte_pktmbuf_free).  The caller holds its own reference on each mbuf it
 * passes (refcnt >= 1) and drops it after nstack_rx_burst / nstack_deliver
 * returns (nstack_mbufs_put); an mbuf's frame must stay in place until its
 * count is 0. */
int nstack_set_rx_inplace(int on, void (*release)(rxg_mbuf *m, void *arg), void *arg);
/* TCP receive coalescing (GRO; the receive side's counterpart of
 * nstack_set_tx_mss).  W == 0 (the default): a connection's segments of a
 * burst make one receive fragment and one ACK each.  W != 0 (bytes, at most
 * RXG_GRO_MAX_WINDOW, else RXG_EINVAL): the GPU runs the coalescing form of
 * the segment sort (RXG_DLV_TCP_GRO, rxg_tune_gro(W); the rule: rxgpu.h, "TCP
 * receive coalescing") and an ESTABLISHED connection's run of k > 1
 * in-sequence PSH|ACK segments makes one receive fragment of the run's bytes —
 * pointing into the held pooled payload buffer when there is one, copied
 * otherwise — and one ACK: rcv_nxt advances by the run's bytes, snd_nxt
 * becomes the run's ack, and the ACK's acknum is rcv_nxt after the run, the
 * ACK that closes the run in the segment-by-segment order.  Every frame of
 * the run is handled with rc 0.  The bytes a connection receives and their
 * order are unchanged; only the count of fragments and ACKs carrying them
 * drops.  Runs of one, and connections on the frame-by-frame path (LISTEN,
 * SYN_RCVD, LAST_ACK), go as before.  A full receive ring drops whole runs
 * (where it would have dropped single segments).  The host-verdict path
 * (nstack_deliver) computes the runs with rxg_tcp_runs_host; the halves and the
 * pipelined nstack_rx_submit / nstack_rx_complete paths honour the option.
 * Not with in-place receive: RXG_EINVAL while nstack_set_rx_inplace is on,
 * and nstack_set_rx_inplace(on) is RXG_EINVAL while W != 0.  nstack_stat(15)
 * counts the segments absorbed into a preceding segment's fragment. */
int nstack_set_rx_gro(uint32_t W);
/* TCP sequence ordering (the third piece beside nstack_set_tx_mss and
 * nstack_set_rx_gro).  on == 0 (the default): a connection's segments of a
 * burst reach its state machine in arrival order.  on != 0: in sequence order
 * (the rule: rxgpu.h, "TCP sequence ordering"): the device paths
 * (nstack_rx_burst, the halves, nstack_rx_submit / nstack_rx_complete) run
 * the ordering form of the segment sort (RXG_DLV_TCP_ORDER), the host-verdict
 * path (nstack_deliver) applies rxg_tcp_order_host to its records before the
 * runs are computed.  Delivery itself follows record order as before.  Works
 * with nstack_set_rx_gro (a train that arrived with a swapped pair coalesces
 * as one run again) and with nstack_set_rx_inplace.  nstack_stat(16) adds up
 * the records that changed position.  A burst delivered frame by frame
 * because the lists changed under it (nstack_stat(5)) keeps arrival order.
 * This reorders what a burst holds; it validates nothing: duplicates are not
 * dropped, a hole is not waited for, and data of segments without PSH is not
 * delivered.  TCP here is not loss-safe with it: that is
 * nstack_set_rx_assemble, below. */
int nstack_set_rx_order(int on);
/* TCP stream assembly: the receive side made loss-safe (the rule and the host
 * rule: rxgpu.h, "TCP stream assembly").  on == 0 (the default): the paths
 * above.  on != 0: a connection's segments of a burst are ordered (as with
 * nstack_set_rx_order, whether that is on or not) and assembled into
 * contiguous byte ranges: duplicates dropped, overlaps trimmed, data counted
 * with or without PSH, a new range at every hole.  Each range is then aligned
 * with the connection's rcv_nxt: bytes below it are passed over, a range that
 * starts above it (data behind a hole) is ignored and answered with an ACK of
 * rcv_nxt.  One receive fragment and one ACK per connection per burst,
 * whatever the segmentation.  The device paths (nstack_rx_burst, the halves,
 * nstack_rx_submit / nstack_rx_complete) set RXG_DLV_TCP_ASSEMBLE, with the
 * pooled payload buffers as before; the host-verdict path (nstack_deliver)
 * applies rxg_tcp_order_host and rxg_tcp_assemble_host and copies from the
 * frames.  A frame delivered on the frame-by-frame path to an ESTABLISHED
 * connection (a burst whose lists changed under it, nstack_stat(5)) is
 * validated as a range of one.  Connections in LISTEN / SYN_RCVD / LAST_ACK
 * keep today's path.  RXG_EINVAL while nstack_set_rx_gro or
 * nstack_set_rx_inplace is on, and those two are RXG_EINVAL while this is on.
 * nstack_stat(19) adds up the payload bytes discarded as already received,
 * nstack_stat(20) the ranges ignored behind a hole.
 * Limits: there is no reassembly queue across bursts (data behind a hole is
 * dropped and must be retransmitted), and the send side still has no
 * retransmission. */
int nstack_set_rx_assemble(int on);
/* The reference's entropy flood detector over the received frames (the rule:
 * rxgpu.h, "Entropy flood detector"; ddos_detect in the reference's I/O loop,
 * before the burst goes into the protocol ring).  on == 0 (the default): off.
 * on != 0: every frame of every burst goes through the detector in arrival
 * order with threshold thresh (RXG_DDOS_DEFAULT_THRESH is the reference's;
 * NaN is RXG_EINVAL): the device paths (nstack_rx_burst, the halves,
 * nstack_rx_submit / nstack_rx_complete) set RXG_DLV_DDOS and the detector
 * runs on the GPU against the context's state; the host-verdict path
 * (nstack_deliver) runs rxg_ddos_host with a state of the stack's own.
 * Detection only: every verdict, delivery and return code is what it is with
 * the option off (the reference exits on a rising alarm; here the application
 * reads nstack_ddos_status and decides).  nstack_stat(17) counts the frames
 * received under alarm, nstack_stat(18) the rises.  nstack_fini resets the
 * option, the state and the status. */
typedef struct nstack_ddos {
    uint64_t frames_seen;  /* frames the detector has seen (the last burst's state) */
    uint64_t rises, falls; /* alarm edges */
    uint64_t alarm_frames; /* frames checked with thresh < D */
    uint64_t undef_frames; /* frames checked on an undefined window */
    double last_stat;      /* D of the last frame seen (NaN: not checked, or undefined) */
    uint32_t alarm;        /* the current alarm state */
    uint32_t _r0;
} nstack_ddos;
int nstack_set_rx_ddos(int on, double thresh);
int nstack_ddos_status(nstack_ddos *out);
/* SYN cookies: listeners that keep no state for a SYN (the rule: rxgpu.h, "SYN
 * cookies").  mode 0 (the default): off, every SYN to a listener creates a
 * tcb in SYN_RCVD as before.  mode 1: on for every listener.  mode 2: on only
 * while the flood detector's alarm is up (RXG_EINVAL unless nstack_set_rx_ddos
 * is on), decided once per burst from the alarm as it stood before the burst.
 * key: the 16 bytes of the hash key (required for mode != 0).
 * With cookies on for a burst, a listener creates no tcb from any SYN.  A SYN
 * that passes the rule is answered by a SYN-ACK whose sequence number is the
 * cookie: its descriptor joins the next nstack_tx_burst (the GPU encoder's
 * descriptor list with nstack_set_tx_encode, the host encoder otherwise; at
 * most 65536 wait, a SYN past that goes unanswered), addressed to the SYN's
 * source MAC with no ARP lookup and no ARP learning.  A handshake ACK whose
 * cookie verifies creates the tcb in ESTABLISHED when it reaches the listener
 * (rcv_nxt = its seq, snd_nxt = its ack), wakes naccept, and is then
 * dispatched on the new tcb, so data or a FIN it carries takes the normal
 * path.  Any other ACK to a listener is counted and ignored.  The counter is
 * CLOCK_MONOTONIC seconds / 64 (a cookie is accepted for
 * RXG_CK_DEFAULT_MAX_AGE counters) unless nstack_syncookie_tick pins it
 * (0xFFFFFFFF: back to the clock).  The device paths (nstack_rx_burst, the
 * halves, nstack_rx_submit / nstack_rx_complete) run K7 with
 * RXG_DLV_SYNCOOKIE; the host-verdict path (nstack_deliver) runs
 * rxg_syncookie_host; the layer keeps the listener mask current (nlisten, the
 * close of a listener).  A frame whose burst result cannot be used (a burst
 * whose lists changed under it, nstack_stat(5)) is judged alone by the same
 * host call.
 * Limit: data segments of a new connection that sit in the same burst as its
 * handshake ACK but ahead of it, or in a burst classified before the new
 * tcb's flow-table insert landed, match the listener, fail the cookie check
 * and are ignored (counted as rejected); the client retransmits them.  No MSS
 * or other option is encoded in the cookie, and no RST answers a bad ACK.
 * nstack_syncookie_stats: {SYNs answered, connections accepted, ACKs rejected,
 * 0}.  nstack_fini resets the option, the counter pin and the counts. */
int nstack_set_syncookies(int mode, const uint8_t key[16]);
int nstack_syncookie_tick(uint32_t t);
int nstack_syncookie_stats(uint64_t out[4]);
/* The L2 responder (the rule: rxgpu.h, "L2 responder"; off by default): with
 * it on, an ARP request for nstack_set_local's address and an ICMP echo request
 * to it are answered by the stack itself (the reference leaves both to the
 * kernel behind KNI, which this project does not forward to), so a peer can
 * resolve the stack and ping it.  RXG_EINVAL while no local address is set.
 * The device paths (nstack_rx_burst, the halves, nstack_rx_submit /
 * nstack_rx_complete) run K8 with RXG_DLV_L2 and room for 256 KiB of answers
 * per burst; the host-verdict path (nstack_deliver) runs rxg_l2_host; a frame
 * whose burst result cannot be used (a burst whose lists changed under it,
 * nstack_stat(5)) is judged alone by the same host call.  The answers are
 * complete frames: copies wait in a queue of at most 1024 frames or 2 MiB of
 * 64-B slots (past either an answer is dropped and counted) and leave at the
 * front of the next nstack_tx_burst, ahead of the UDP and TCP walks, under its
 * max_frames and cap_bytes (what does not fit stays queued), with cksum 0 or
 * not and with nstack_set_tx_encode on or off: the encoder gets the room and
 * the frame slots behind them.  ARP learning is what it is without the
 * option.  Limits: one local address, no IPv4 options, no fragments, no rate
 * limit beyond the per-burst room and the queue.  nstack_stat(21) counts the
 * ARP answers queued, (22) the echo answers queued, (23) the answers dropped
 * for room, (24) the echo requests with a bad checksum or a cut capture.
 * nstack_fini resets the option, the queue and the counts. */
int nstack_set_l2_respond(int on);
/* Items the application has read (fragments, datagram batches) are handed
 * back to the protocol thread and freed by its next nstack_rx_burst (while
 * that burst is on the GPU) / nstack_tx_burst / nstack_deliver call (or
 * nstack_reclaim, a protocol-thread call): in place, a frame's mbuf count
 * reaches 0 there.  A thread that made
 * one of those calls frees what it reads at once. */
void nstack_reclaim(void);
/* drop one reference on each of n mbufs (rte_pktmbuf_free of a burst):
 * release(m, arg) of nstack_set_rx_inplace for each whose count reaches 0 */
void nstack_mbufs_put(rxg_mbuf *const *m, uint32_t n);

/* Where the last nstack_rx_burst's time went, in ms: [0] gather of the mbufs
 * into pinned staging (host), [1] copy in, [2] classify (K1), [3] UDP
 * compaction + TCP segment sort (K3 + K4), [4] copy out of their results
 * (device, HIP events), [5] the library calls (submit + wait, host clock),
 * then host delivery: [6] UDP batches to the sockets, [7] TCP connections
 * from the segment sort, [8] the frame-by-frame loop over the rest, [9] the
 * whole nstack_rx_burst; [10] segments sorted, [11] datagrams compacted.  A
 * burst run as two halves adds up both halves' phases, so [1]-[4] may exceed
 * the wall time they took.  A protocol-thread call: like nstack_rx_burst it
 * takes the stack's lock ahead of an application loop (nstack_drain_all). */
int nstack_last_burst_phases(float ms[12]);
/* Bursts of at least 2 * min_half frames run as two halves, both on the GPU
 * at once (rxg_deliver_submit twice: the second half's copy in overlaps the
 * first half's copy out, and the host delivers the first half while the
 * second is on the GPU); 0 (the default) = never.  Measured on MI355X: no
 * gain for 16K-32K-frame bursts, hence off. */
int nstack_set_halves(uint32_t min_half);

/* counters: 0 = UDP datagrams delivered, 1 = dropped (a receive ring full),
 * 2 = TCP segments dispatched to the state machine, 3 = frames handed to KNI,
 * 4 = TCP fragments (payload or EOF) queued for nrecv, 5 = bursts (or burst
 * halves) delivered frame by frame because the lists changed while they were
 * on the GPU, 6 = TCP payload bytes copied on the host (the sorted segments'
 * payloads are otherwise queued in place, in a pooled pinned buffer the
 * library holds until the application has read them; copied when no pooled
 * buffer was free, or for a segment cut short by its capture), 7 = fragment
 * batches now queued that hold such a buffer (read without the lock); 8-10 =
 * nstack_drain_all's time in ns (read without the lock): waiting for the
 * id maps' lock (never the stack's), stepping aside for the protocol thread
 * (0 since round 5: nothing to step aside from), reading out what it took
 * from the blocks (outside every lock but the block's own); 11 = bursts
 * that waited for a pooled payload buffer while an application thread was
 * draining (at most 20 ms each; the stack's lock released meanwhile); 12 =
 * bursts delivered (nstack_rx_burst, nstack_deliver), read without any lock: a
 * polling application that reads a value it has not seen finds that burst's
 * items in its next nstack_drain_all (bumped with release order after the
 * deliveries, read with acquire); 13 = frames produced by the TX encoder
 * (nstack_set_tx_encode); 14 = fragments sent as more than one frame in a
 * pass (nstack_set_tx_mss); 15 = segments absorbed into a preceding segment's
 * receive fragment (nstack_set_rx_gro); 16 = segment records moved by sequence
 * ordering (nstack_set_rx_order); 17 = frames received under the flood detector's
 * alarm, 18 = its rises (nstack_set_rx_ddos); 19 = payload bytes discarded as
 * already received, 20 = streams ignored behind a hole
 * (nstack_set_rx_assemble); 21-24 = the L2 responder's ARP answers queued,
 * echo answers queued, answers dropped for room, echo requests with a bad
 * checksum or a cut capture (nstack_set_l2_respond); 25 = datagrams sent as
 * IPv4 fragments (nstack_set_tx_mtu).  Counter 1 also counts TX items dropped (a
 * send ring full, or a datagram too long for a frame). */
uint64_t nstack_stat(int which);

#ifdef __cplusplus
}
#endif
#endif
