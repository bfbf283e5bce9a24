/*
 * refrun_main.c — driver that runs the reference's own compiled code
 * (build/tcp.o, build/udp.o, build/common.o, linked with refrun_stubs.c)
 * on a binary case file and writes a binary result file.
 *
 * TEST INFRASTRUCTURE ONLY.  Usage: refrun CASEFILE RESULTFILE
 *
 * Both files are sequences of records {u32 op, u32 len, payload[len]},
 * little-endian, in order.  The tables a case file builds live for the whole
 * run; tests/ref_bind.py writes and parses the records.
 *
 *  op  payload in                                  payload out
 *  1   UDPSOCK  ip u32, port u16, proto u8, pad u8   (none)
 *  2   TCB      sip,dip u32; sport,dport u16;        how_used u32
 *               status u32; how u32
 *               how 0: nsocket/nbind(/nlisten)  1: hand-built 160-B node
 *               how 2: a SYN through tcp_process to a listener (falls back to 1)
 *  3   CKSUM    align u32; bytes                     raw, udptcp, ipv4 u16
 *  4   LKUDP    dip u32, port u16, proto u8, pad     creation index u32
 *  5   LKTCP    sip,dip u32; sport,dport u16         creation index u32
 *  6   RX       flags u32 (1: nrecvfrom), delta u32; rx record (below)
 *               frame bytes
 *  7   TX       frame bytes                          ipck,l4ck u16; has_ip,has_l4 u8
 *
 * rx record: rc i32 (1: neither function called), l4_cksum u16 (field zeroed),
 * family u8 (17 / 6 / 0), delivered u8, match u32 (creation index of the
 * block the lookup returns, ~0 for none); if delivered, the ring slot's
 * offload: length, sport, dport, pad u16; sip, dip u32; protocol i32;
 * copied_equal u32 (the bytes copied equal frame[42 : 42+length-8] of the
 * zero-extended frame); then with flag 1, for a caller buffer of
 * length-delta, length and length+delta bytes (the datagram is delivered
 * again for each): buflen u32, ret i64, sin_addr u32, sin_port u16, pad u16,
 * n u32, bytes[n]; and the second read that takes a re-queued rest:
 * ret2 i64 (-100: none was needed), n2 u32, bytes[n2].
 *
 * Exit status: 70 the reference called rte_exit, 71 it panicked (both in
 * refrun_stubs.c), 72 bad case file, 73 a state check of this driver failed.
 *
 * Struct offsets are the DWARF facts of SURVEY.md §8(a).  Every frame is laid
 * at the start of a freshly zeroed buffer of 65,535 + 128 bytes, so what the
 * reference reads past the capture is zeros (the project's RXG_F_TRUNC rule).
 */
#include <netinet/in.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/types.h>

#define EXIT_FORMAT 72
#define EXIT_STATE 73

#define NONE 0xFFFFFFFFu
#define BIG (65535 + 128)
#define MAXBLK 4096

/* the reference's compiled code */
extern int udp_process(void *mbuf);
extern int tcp_process(void *mbuf);
extern void *get_hostinfo_fromip_port(uint32_t dip, uint16_t port, unsigned char proto);
extern void *tcp_stream_search(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport);
extern void *tcpInstance(void);
extern int nsocket(int domain, int type, int protocol);
extern int nbind(int fd, const struct sockaddr *addr, socklen_t len);
extern int nlisten(int fd, int backlog);
extern ssize_t nrecvfrom(int fd, void *buf, size_t len, int flags, struct sockaddr *src,
                         socklen_t *alen);
extern uint16_t rte_raw_cksum(const void *buf, size_t len);              /* tcp.o, globalized */
extern uint16_t rte_ipv4_udptcp_cksum(const void *ip, const void *l4);   /* tcp.o, globalized */
extern uint16_t refobj_rte_ipv4_cksum(const void *ip);                   /* udp.o, renamed */
extern void *rte_ring_create(const char *name, unsigned count, int socket_id, unsigned flags);

extern void *g_pstTcpTbl, *g_pstHost;

/* struct localhost (144 B) / struct tcp_stream (160 B) / tcp_table / rte_ring / offload */
enum { H_FD = 0, H_PROTO = 16, H_RCVBUF = 32, H_NEXT = 48 };
enum { T_FD = 0, T_DIP = 4, T_DPORT = 14, T_PROTO = 16, T_SPORT = 18, T_SIP = 20, T_STATUS = 32,
       T_SNDBUF = 40, T_RCVBUF = 48, T_PREV = 56, T_NEXT = 64, T_SIZE = 160 };
enum { TBL_SET = 8 };
enum { R_MASK = 52, R_PROD_TAIL = 132, R_CONS_TAIL = 260, R_SLOTS = 384 };
enum { O_SIP = 0, O_DIP = 4, O_SPORT = 8, O_DPORT = 10, O_PROTO = 12, O_DATA = 16, O_LEN = 24 };
enum { M_BUF = 0, M_DATAOFF = 16, M_REFCNT = 18, M_NBSEGS = 20, M_PKTLEN = 36, M_DATALEN = 40,
       M_SIZE = 128 };

static uint8_t *udp_nodes[MAXBLK], *tcb_nodes[MAXBLK];
static uint32_t n_udp, n_tcb;

static FILE *fout;

static void die(int code, const char *what) {
    fprintf(stderr, "refrun: %s\n", what);
    exit(code);
}

static uint32_t g32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint16_t g16(const uint8_t *p) { uint16_t v; memcpy(&v, p, 2); return v; }
static void *gptr(const uint8_t *p) { void *v; memcpy(&v, p, 8); return v; }
static void pptr(uint8_t *p, const void *v) { memcpy(p, &v, 8); }

/* growing output payload */
static uint8_t *ob;
static size_t on, ocap;
static void oput(const void *p, size_t n) {
    if (on + n > ocap) {
        ocap = (on + n) * 2 + 256;
        ob = (uint8_t *)realloc(ob, ocap);
        if (!ob) die(EXIT_STATE, "out of memory");
    }
    memcpy(ob + on, p, n);
    on += n;
}
static void o8(uint8_t v) { oput(&v, 1); }
static void o16(uint16_t v) { oput(&v, 2); }
static void o32(uint32_t v) { oput(&v, 4); }
static void o64(int64_t v) { oput(&v, 8); }
static void oflush(uint32_t op) {
    uint32_t h[2] = {op, (uint32_t)on};
    if (fwrite(h, 4, 2, fout) != 2 || (on && fwrite(ob, 1, on, fout) != on))
        die(EXIT_STATE, "short write");
    on = 0;
}

static uint8_t **tcb_head(void) { return (uint8_t **)((uint8_t *)tcpInstance() + TBL_SET); }

static uint32_t index_of(uint8_t *const *nodes, uint32_t n, const void *p) {
    if (!p) return NONE;
    for (uint32_t i = 0; i < n; i++)
        if (nodes[i] == p) return i;
    die(EXIT_STATE, "lookup returned a block the driver did not create");
    return NONE;
}

/* a frame at the start of a fresh zeroed buffer, and a fake mbuf over it:
 * refcnt 2 and next NULL make rte_pktmbuf_free a plain decrement */
static uint8_t *fresh_frame(const uint8_t *f, uint32_t cap) {
    uint8_t *b = (uint8_t *)calloc(1, BIG);
    if (!b) die(EXIT_STATE, "out of memory");
    memcpy(b, f, cap);
    return b;
}
static uint8_t *fake_mbuf(uint8_t *frame, uint32_t cap) {
    uint8_t *m = (uint8_t *)aligned_alloc(64, M_SIZE);
    memset(m, 0, M_SIZE);
    pptr(m + M_BUF, frame);
    uint16_t two = 2, one = 1, dl = (uint16_t)cap;
    memcpy(m + M_REFCNT, &two, 2);
    memcpy(m + M_NBSEGS, &one, 2);
    memcpy(m + M_PKTLEN, &cap, 4);
    memcpy(m + M_DATALEN, &dl, 2);
    return m;
}


static int run_frame(int (*fn)(void *), const uint8_t *f, uint32_t cap) {
    uint8_t *b = fresh_frame(f, cap);
    uint8_t *m = fake_mbuf(b, cap);
    int rc = fn(m); /* neither function keeps a pointer into the frame */
    free(m);
    free(b);
    return rc;
}

/* ---- table building ---------------------------------------------------- */

static void op_udpsock(const uint8_t *p, uint32_t len) {
    if (len != 8 || n_udp >= MAXBLK) die(EXIT_FORMAT, "bad UDPSOCK");
    int fd = nsocket(AF_INET, SOCK_DGRAM, 0);
    if (fd < 0) die(EXIT_STATE, "nsocket failed");
    struct sockaddr_in a;
    memset(&a, 0, sizeof(a));
    a.sin_family = AF_INET;
    a.sin_port = g16(p + 4);
    a.sin_addr.s_addr = g32(p);
    /* the new socket is the list head, which get_hostinfo_fromfd finds first */
    if (nbind(fd, (struct sockaddr *)&a, sizeof(a)) != 0) die(EXIT_STATE, "nbind failed");
    uint8_t *h = (uint8_t *)g_pstHost;
    if (p[6] != 17) h[H_PROTO] = p[6]; /* no API sets another protocol: patched */
    udp_nodes[n_udp++] = h;
}

static uint8_t *handbuilt_tcb(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport,
                              uint32_t status) {
    uint8_t *s = (uint8_t *)calloc(1, T_SIZE);
    int32_t fd = -1;
    memcpy(s + T_FD, &fd, 4);
    memcpy(s + T_DIP, &dip, 4);
    memcpy(s + T_DPORT, &dport, 2);
    s[T_PROTO] = 6;
    memcpy(s + T_SPORT, &sport, 2);
    memcpy(s + T_SIP, &sip, 4);
    memcpy(s + T_STATUS, &status, 4);
    pptr(s + T_SNDBUF, rte_ring_create("s", 1024, 0, 0));
    pptr(s + T_RCVBUF, rte_ring_create("r", 1024, 0, 0));
    uint8_t **head = tcb_head(); /* head insert, as the reference's list macro does */
    pptr(s + T_NEXT, *head);
    if (*head) pptr(*head + T_PREV, s);
    *head = s;
    return s;
}

static uint8_t *syn_tcb(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport) {
    uint8_t f[54];
    memset(f, 0, sizeof(f));
    f[12] = 0x08;
    f[14] = 0x45;
    f[17] = 40; /* total_length */
    f[22] = 64;
    f[23] = 6;
    memcpy(f + 26, &sip, 4);
    memcpy(f + 30, &dip, 4);
    memcpy(f + 34, &sport, 2);
    memcpy(f + 36, &dport, 2);
    f[46] = 0x50;
    f[47] = 0x02; /* SYN */
    uint16_t c = rte_ipv4_udptcp_cksum(f + 14, f + 34);
    memcpy(f + 50, &c, 2);
    uint8_t **head = tcb_head();
    uint8_t *before = *head;
    int rc = run_frame(tcp_process, f, sizeof(f));
    uint8_t *s = *head;
    if (rc != 0 || s == before || !s || gptr(s + T_NEXT) != before) return NULL;
    if (g32(s + T_SIP) != sip || g32(s + T_DIP) != dip || g16(s + T_SPORT) != sport ||
        g16(s + T_DPORT) != dport)
        die(EXIT_STATE, "SYN created an unexpected block");
    return s;
}

static void op_tcb(const uint8_t *p, uint32_t len) {
    if (len != 20 || n_tcb >= MAXBLK) die(EXIT_FORMAT, "bad TCB");
    uint32_t sip = g32(p), dip = g32(p + 4), status = g32(p + 12), how = g32(p + 16);
    uint16_t sport = g16(p + 8), dport = g16(p + 10);
    uint8_t *s = NULL;
    if (how == 0) {
        if (sip || sport || status > 1) die(EXIT_FORMAT, "TCB how 0 needs sip = sport = 0");
        int fd = nsocket(AF_INET, SOCK_STREAM, 0);
        if (fd < 0) die(EXIT_STATE, "nsocket failed");
        struct sockaddr_in a;
        memset(&a, 0, sizeof(a));
        a.sin_family = AF_INET;
        a.sin_port = dport;
        a.sin_addr.s_addr = dip;
        /* get_hostinfo_fromfd never leaves the UDP list once it holds two
         * sockets (common.c:116); hide that list while the fd is looked up */
        void *hosts = g_pstHost;
        g_pstHost = NULL;
        int r = nbind(fd, (struct sockaddr *)&a, sizeof(a));
        if (r == 0 && status == 1) r = nlisten(fd, 8);
        g_pstHost = hosts;
        if (r != 0) die(EXIT_STATE, "nbind/nlisten failed");
        s = *tcb_head();
    } else if (how == 2) {
        s = syn_tcb(sip, dip, sport, dport);
        if (s) {
            /* the handler leaves SYN_RCVD; lookups only tell LISTEN from the rest */
            if (status == 1) die(EXIT_FORMAT, "TCB how 2 cannot make a listener");
            memcpy(s + T_STATUS, &status, 4);
        } else {
            how = 1;
        }
    }
    if (how == 1) s = handbuilt_tcb(sip, dip, sport, dport, status);
    if (!s) die(EXIT_FORMAT, "bad TCB how");
    tcb_nodes[n_tcb++] = s;
    o32(how);
    oflush(2);
}

/* ---- cases -------------------------------------------------------------- */

static void op_cksum(const uint8_t *p, uint32_t len) {
    if (len < 4) die(EXIT_FORMAT, "bad CKSUM");
    uint32_t align = g32(p) & 63, n = len - 4;
    if (n > 65535) die(EXIT_FORMAT, "CKSUM too long");
    uint8_t *b = (uint8_t *)calloc(1, BIG + 64);
    uint8_t *buf = b + align;
    memcpy(buf, p + 4, n);
    o16(rte_raw_cksum(buf, n));
    o16(rte_ipv4_udptcp_cksum(buf, buf + 20));
    o16(refobj_rte_ipv4_cksum(buf));
    oflush(3);
    free(b);
}

static void op_lkudp(const uint8_t *p, uint32_t len) {
    if (len != 8) die(EXIT_FORMAT, "bad LKUDP");
    o32(index_of(udp_nodes, n_udp, get_hostinfo_fromip_port(g32(p), g16(p + 4), p[6])));
    oflush(4);
}

static void op_lktcp(const uint8_t *p, uint32_t len) {
    if (len != 12) die(EXIT_FORMAT, "bad LKTCP");
    o32(index_of(tcb_nodes, n_tcb,
                 tcp_stream_search(g32(p), g32(p + 4), g16(p + 8), g16(p + 10))));
    oflush(5);
}

static int ring_count(const uint8_t *r) { return g32(r + R_PROD_TAIL) != g32(r + R_CONS_TAIL); }

static void drop_new_tcbs(uint8_t *before) {
    /* a SYN that reaches a listener makes the LISTEN handler add a block;
     * take it off again so that every rx case sees the same tables */
    uint8_t **head = tcb_head();
    if (*head != before) {
        *head = before;
        if (before) pptr(before + T_PREV, NULL);
    }
}

static void op_rx(const uint8_t *p, uint32_t len) {
    if (len < 8) die(EXIT_FORMAT, "bad RX");
    const uint32_t flags = g32(p), delta = g32(p + 4), cap = len - 8;
    const uint8_t *f = p + 8;
    if (cap > 65535) die(EXIT_FORMAT, "RX frame too long");

    uint8_t *z = fresh_frame(f, cap); /* the zero-extended view, kept unchanged */
    /* the demux rule of the reference's receive loop, restated: ethertype
     * bytes 08 00, then protocol 17 -> udp_process, 6 -> tcp_process */
    uint8_t fam = 0;
    if (z[12] == 0x08 && z[13] == 0x00 && (z[23] == 17 || z[23] == 6)) fam = z[23];

    int32_t rc = 1; /* everything else goes to the kernel interface */
    uint16_t l4 = 0;
    uint32_t match = NONE;
    uint8_t delivered = 0;
    uint8_t *host = NULL;

    if (fam) {
        uint8_t *c = fresh_frame(f, cap);
        uint32_t hole = fam == 17 ? 40 : 50;
        c[hole] = c[hole + 1] = 0;
        l4 = rte_ipv4_udptcp_cksum(c + 14, c + 34);
        free(c);
    }
    if (fam == 17) {
        host = (uint8_t *)get_hostinfo_fromip_port(g32(z + 30), g16(z + 36), 17);
        match = index_of(udp_nodes, n_udp, host);
        if (host && ring_count((uint8_t *)gptr(host + H_RCVBUF)))
            die(EXIT_STATE, "receive ring not empty before the case");
        rc = run_frame(udp_process, f, cap);
        delivered = rc == 0;
    } else if (fam == 6) {
        match = index_of(tcb_nodes, n_tcb,
                         tcp_stream_search(g32(z + 26), g32(z + 30), g16(z + 34), g16(z + 36)));
        uint8_t *before = *tcb_head();
        rc = run_frame(tcp_process, f, cap);
        drop_new_tcbs(before);
    }
    o32((uint32_t)rc);
    o16(l4);
    o8(fam);
    o8(delivered);
    o32(match);

    if (delivered) {
        uint8_t *ring = (uint8_t *)gptr(host + H_RCVBUF);
        if (!ring_count(ring)) die(EXIT_STATE, "rc 0 but nothing queued");
        uint8_t *o = (uint8_t *)gptr(ring + R_SLOTS + 8 * (g32(ring + R_CONS_TAIL) & g32(ring + R_MASK)));
        uint16_t olen = g16(o + O_LEN);
        const uint8_t *data = (const uint8_t *)gptr(o + O_DATA);
        o16(olen);
        o16(g16(o + O_SPORT));
        o16(g16(o + O_DPORT));
        o16(0);
        o32(g32(o + O_SIP));
        o32(g32(o + O_DIP));
        o32(g32(o + O_PROTO));
        o32(olen >= 8 && memcmp(data, z + 42, (size_t)olen - 8) == 0);

        int32_t fd;
        memcpy(&fd, host + H_FD, 4);
        const size_t want[3] = {olen > delta ? olen - delta : 0, olen, (size_t)olen + delta};
        uint8_t *ub = (uint8_t *)malloc(BIG);
        for (int k = 0; k < 3; k++) {
            if (!(flags & 1)) break;
            if (k > 0) { /* each read consumes the datagram: deliver it again */
                if (run_frame(udp_process, f, cap) != 0) die(EXIT_STATE, "redelivery failed");
            }
            for (int pass = 0; pass < 2; pass++) {
                struct sockaddr_in src;
                memset(&src, 0, sizeof(src));
                memset(ub, 0xCC, BIG);
                /* get_hostinfo_fromfd only reaches the first two sockets of
                 * the list: make this one the head for the call */
                void *hosts = g_pstHost;
                g_pstHost = host;
                ssize_t r = nrecvfrom(fd, ub, pass == 0 ? want[k] : (size_t)65535 + 64, 0,
                                      (struct sockaddr *)&src, NULL);
                g_pstHost = hosts;
                if (pass == 0) {
                    o32((uint32_t)want[k]);
                    o64(r);
                    o32(src.sin_addr.s_addr);
                    o16(src.sin_port);
                    o16(0);
                } else {
                    o64(r);
                }
                uint32_t nb = r > 0 ? (uint32_t)r : 0;
                o32(nb);
                oput(ub, nb);
                if (!ring_count(ring)) { /* whole datagram taken: no second pass */
                    if (pass == 0) {
                        o64(-100);
                        o32(0);
                    }
                    break;
                }
                if (pass == 1) die(EXIT_STATE, "datagram not drained");
            }
        }
        if (!(flags & 1)) { /* leave the ring empty for the next case */
            void *hosts = g_pstHost;
            g_pstHost = host;
            struct sockaddr_in src;
            nrecvfrom(fd, ub, (size_t)65535 + 64, 0, (struct sockaddr *)&src, NULL);
            g_pstHost = hosts;
        }
        free(ub);
    }
    oflush(6);
    free(z);
}

static void op_tx(const uint8_t *p, uint32_t len) {
    if (len > 65535) die(EXIT_FORMAT, "TX frame too long");
    uint8_t *b = fresh_frame(p, len);
    uint16_t ipck = 0, l4ck = 0;
    uint8_t has_ip = 0, has_l4 = 0;
    if (b[12] == 0x08 && b[13] == 0x00) {
        /* the encoders' order, restated: clear and fill the header checksum,
         * then clear and fill the L4 checksum over the finished header */
        uint8_t *ip = b + 14;
        ip[10] = ip[11] = 0;
        ipck = refobj_rte_ipv4_cksum(ip);
        memcpy(ip + 10, &ipck, 2);
        has_ip = 1;
        if (ip[9] == 17 || ip[9] == 6) {
            uint32_t hole = ip[9] == 17 ? 40 : 50;
            b[hole] = b[hole + 1] = 0;
            l4ck = rte_ipv4_udptcp_cksum(ip, ip + 20);
            has_l4 = 1;
        }
    }
    o16(ipck);
    o16(l4ck);
    o8(has_ip);
    o8(has_l4);
    oflush(7);
    free(b);
}

int main(int argc, char **argv) {
    if (argc != 3) die(EXIT_FORMAT, "usage: refrun CASEFILE RESULTFILE");
    FILE *fin = fopen(argv[1], "rb");
    if (!fin) die(EXIT_FORMAT, "cannot open case file");
    fseek(fin, 0, SEEK_END);
    long sz = ftell(fin);
    fseek(fin, 0, SEEK_SET);
    uint8_t *in = (uint8_t *)malloc((size_t)sz + 1);
    if (!in || fread(in, 1, (size_t)sz, fin) != (size_t)sz) die(EXIT_FORMAT, "cannot read case file");
    fclose(fin);
    fout = fopen(argv[2], "wb");
    if (!fout) die(EXIT_FORMAT, "cannot open result file");

    size_t pos = 0;
    while (pos + 8 <= (size_t)sz) {
        uint32_t op = g32(in + pos), len = g32(in + pos + 4);
        pos += 8;
        if (pos + len > (size_t)sz) die(EXIT_FORMAT, "truncated record");
        const uint8_t *p = in + pos;
        switch (op) {
        case 1: op_udpsock(p, len); break;
        case 2: op_tcb(p, len); break;
        case 3: op_cksum(p, len); break;
        case 4: op_lkudp(p, len); break;
        case 5: op_lktcp(p, len); break;
        case 6: op_rx(p, len); break;
        case 7: op_tx(p, len); break;
        default: die(EXIT_FORMAT, "unknown op");
        }
        pos += len;
    }
    if (pos != (size_t)sz) die(EXIT_FORMAT, "trailing bytes");
    if (fclose(fout) != 0) die(EXIT_STATE, "close failed");
    return 0;
}
