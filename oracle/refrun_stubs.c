/*
 * refrun_stubs.c — what the reference's prebuilt objects need from DPDK and
 * from netfamily.o, written from SURVEY.md §8(c) and the DWARF facts of §8(a).
 *
 * TEST INFRASTRUCTURE ONLY.  Linked with the reference's own tcp.o, udp.o and
 * common.o into oracle/_ref/refrun (never committed).  Nothing here restates
 * reference logic: these are the environment's answers, and two of them decide
 * results the tests then record:
 *   - rte_malloc returns NULL for size 0 (as DPDK 19.11's does) and for sizes
 *     above 1 GiB (the wrapped size_t of dgram_len < 8): this is what makes
 *     udp_process return -2 for dgram_len <= 8;
 *   - rte_malloc pads every block with 64 zero bytes, so nrecvfrom's 8-byte
 *     read past the payload buffer (common.c:558-559) sees zeros.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define EXIT_RTE_EXIT 70
#define EXIT_RTE_PANIC 71

__thread unsigned per_lcore__lcore_id;
__thread int per_lcore__rte_errno;
char rte_mempool_ops_table[65536] __attribute__((aligned(64)));

/* globals that netfamily.o defines in the reference program */
void *g_pstTcpTbl, *g_pstHost, *g_pstArpTbl, *g_pstRingIns;
unsigned char g_ucFdTable[1024];
unsigned char g_stCpuMac[6] = {0x02, 0x00, 0x00, 0x00, 0x00, 0x01};
unsigned char g_aucDefaultArpMac[6] = {0xff, 0xff, 0xff, 0xff, 0xff, 0xff};

#define MALLOC_PAD 64
#define MALLOC_MAX ((size_t)1 << 30)

void *rte_malloc(const char *type, size_t size, unsigned align) {
    (void)type;
    (void)align;
    if (size == 0 || size > MALLOC_MAX) return NULL;
    return calloc(1, size + MALLOC_PAD);
}

void rte_free(void *p) { free(p); }

void rte_exit(int code, const char *fmt, ...) {
    (void)code;
    (void)fmt;
    _exit(EXIT_RTE_EXIT);
}

void __rte_panic(const char *func, const char *fmt, ...) {
    (void)func;
    (void)fmt;
    _exit(EXIT_RTE_PANIC);
}

unsigned rte_socket_id(void) { return 0; }

/* struct rte_ring of DPDK 19.11 as the objects' inlined enqueue/dequeue see
 * it: flags@32 size@48 mask@52 capacity@56, prod {head@128 tail@132
 * single@136}, cons {head@256 tail@260 single@264}, slots from +384. */
#define RING_HDR 384
void *rte_ring_create(const char *name, unsigned count, int socket_id, unsigned flags) {
    (void)socket_id;
    if (count == 0 || (count & (count - 1))) return NULL;
    size_t bytes = RING_HDR + (size_t)count * 8;
    bytes = (bytes + 127) & ~(size_t)127;
    uint8_t *r = (uint8_t *)aligned_alloc(128, bytes);
    if (!r) return NULL;
    memset(r, 0, bytes);
    if (name) strncpy((char *)r, name, 31);
    uint32_t v;
    v = flags;
    memcpy(r + 32, &v, 4);
    v = count;
    memcpy(r + 48, &v, 4);
    v = count - 1;
    memcpy(r + 52, &v, 4);
    memcpy(r + 56, &v, 4);
    v = (flags & 1u) ? 1 : 0; /* RING_F_SP_ENQ */
    memcpy(r + 136, &v, 4);
    v = (flags & 2u) ? 1 : 0; /* RING_F_SC_DEQ */
    memcpy(r + 264, &v, 4);
    return r;
}

void rte_ring_free(void *r) { free(r); }

/* the reference prints per packet; keep stdout silent (diagnostics of the
 * driver go to stderr) */
int printf(const char *fmt, ...) {
    (void)fmt;
    return 0;
}
int puts(const char *s) {
    (void)s;
    return 0;
}
int putchar(int c) { return c; }
