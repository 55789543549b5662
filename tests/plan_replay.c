/* SPDX-License-Identifier: GPL-2.0 */
/*
 * plan_replay — the launch plan (xdp-tools_amd/csrc/xfg_plan.c) over recorded
 * cases, on the CPU: tests/test_plan.py.
 *
 * Input lines of key=value pairs (tests/golden/plan_cases.txt):
 *   dev feat=F ncu=N thr=<18 ints> occ=<288 ints>
 *       a device's tables for program F; holds for the cases of F after it
 *   case id=I feat=F n= stride= ... [XFG_<knob>=value ...] | <outputs>
 *       a launch's plan inputs; what follows " | " is not read here
 * Output: one line "id=I <outputs>" a case, in the recorded form.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xfg_plan.h"

struct dev {
	int ncu, thr[XFG_OCC_KINDS][2], occ[XFG_OCC_KINDS][2][16];
};

static void ints(const char *v, int *out, int n)
{
	for (int i = 0; i < n; i++) {
		out[i] = (int)strtol(v, (char **)&v, 10);
		if (*v == ',')
			v++;
	}
}

int main(int argc, char **argv)
{
	static struct dev devs[128];
	static char line[1 << 14];
	FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!f) {
		perror(argv[1]);
		return 2;
	}
	while (fgets(line, sizeof(line), f)) {
		const int is_dev = !strncmp(line, "dev ", 4);
		if (!is_dev && strncmp(line, "case ", 5))
			continue;
		struct xfg_plan_in in = { 0 };
		struct xfg_knobs k;
		struct dev dv = { 0 };
		char id[64] = "?";
		int have_knobs = 0;
		xfg_knobs_init(&k);
		for (char *sp, *t = strtok_r(line + (is_dev ? 4 : 5), " \n", &sp); t && strcmp(t, "|");
		     t = strtok_r(NULL, " \n", &sp)) {
			char *v = strchr(t, '=');
			if (!v) {
				fprintf(stderr, "no value: %s\n", t);
				return 2;
			}
			*v++ = 0;
			const uint64_t u = strtoull(v, NULL, 0);
			if (!strcmp(t, "id"))
				snprintf(id, sizeof(id), "%s", v);
			else if (!strcmp(t, "feat")) in.feat = (uint32_t)u;
			else if (!strcmp(t, "ncu")) dv.ncu = (int)u;
			else if (!strcmp(t, "thr")) ints(v, &dv.thr[0][0], XFG_OCC_KINDS * 2);
			else if (!strcmp(t, "occ")) ints(v, &dv.occ[0][0][0], XFG_OCC_KINDS * 32);
			else if (!strcmp(t, "n")) in.n = u;
			else if (!strcmp(t, "stride")) in.stride = (uint32_t)u;
			else if (!strcmp(t, "offs")) in.offsets = (int)u;
			else if (!strcmp(t, "al16")) in.aligned16 = (int)u;
			else if (!strcmp(t, "descs")) in.descs = (int)u;
			else if (!strcmp(t, "hwin")) in.hwin = (int)u;
			else if (strlen(t) == 2 && strchr("cfbs", t[0]) && strchr("46e", t[1])) {
				const int m = t[1] == '4' ? 0 : t[1] == '6' ? 1 : 2;   /* c4 f4 b4 s4, ..6, ..e */
				switch (t[0]) {
				case 'c': in.map[m].count = (uint32_t)u; break;
				case 'f': in.map[m].fmask = (uint32_t)u; break;
				case 'b': in.map[m].bloom_words = (uint32_t)u; break;
				default: in.map[m].nslots = (uint32_t)u; break;
				}
			}
			else if (!strcmp(t, "fd4")) in.flags_differ4 = (uint32_t)u;
			else if (!strcmp(t, "ports")) in.port_count = (uint32_t)u;
			else if (!strcmp(t, "ptab")) in.port_tab_ok = (int)u;
			else if (!strcmp(t, "win")) in.ctx_window = (uint32_t)u;
			else if (!strcmp(t, "qtmin")) in.qt_min_keys = (uint32_t)u;
			else if (!strcmp(t, "dmin")) in.descs_min = (uint32_t)u;
			else if (!strcmp(t, "ekok")) in.ek_ok = (int)u;
			else if (!strcmp(t, "qt_n")) in.qt_n = (uint32_t)u;
			else if (!strcmp(t, "qt_live")) in.qt_live = (uint32_t)u;
			else if (!strcmp(t, "qt_nimg")) in.qt_nimg = (uint32_t)u;
			else if (!strcmp(t, "qt_bits")) in.qt_bits = (uint32_t)u;
			else if (!strcmp(t, "ek_slots")) in.ek_slots = (uint32_t)u;
			else if (!xfg_knobs_set(&k, t, v)) have_knobs = 1;
			else {
				fprintf(stderr, "unknown key: %s\n", t);
				return 2;
			}
		}
		if (is_dev) {
			devs[in.feat & 127] = dv;
			continue;
		}
		const struct dev *d = &devs[in.feat & 127];
		if (!d->ncu) {
			fprintf(stderr, "case %s: no dev line for feat %u\n", id, in.feat);
			return 2;
		}
		in.ncu = d->ncu;
		in.occ = d->occ;
		in.thr = d->thr;
		in.knobs = have_knobs ? &k : NULL;
		struct xfg_wants w;
		struct xfg_plan p;
		xfg_plan_wants(&in, &w);
		xfg_plan(&in, &p);
		printf("id=%s kind=%d window=%u pipe=%u dense=%u km=%u v6d=%u v6p=%u split=%u ek=%d qt=%d"
		       " dcnt=%u bl_lds=%u bl_off=%u,%u,%u grid=%u grid_parse=%u defer_cap=%u defer_sep=%u"
		       " defer_grid=%u logs=%d log_span=%u log_hist=%u pwide=%u pcap=%u K=%u cw=%d qt_dyn=%u"
		       " want_ek=%d want_qt=%u pbuf_bytes=%" PRIu64 " pfill_bytes=%" PRIu64 " defer_bytes=%" PRIu64
		       " qt_hits_bytes=%" PRIu64 "\n",
		       id, p.kind, p.window, p.pipe, p.dense, p.km, p.v6d, p.v6p, p.split, p.use_ek, p.use_qt,
		       p.dcnt, p.bl_lds, p.bl_off[0], p.bl_off[1], p.bl_off[2], p.grid, p.grid_parse, p.defer_cap,
		       p.defer_sep, p.defer_grid, p.logs, p.log_span, p.log_hist, p.pwide, p.pcap, p.K, p.cw,
		       p.qt_dyn, w.ek, w.qt_live, p.bytes.pbuf, p.bytes.pfill, p.bytes.defer, p.bytes.qt_hits);
	}
	return 0;
}
