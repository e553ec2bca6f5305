// pv_carry.h -- what the tuned power-of-two families (pv_kernels_v2.h, _v3.h, _sub.h, _eo.h; _team.h through _eo.h) share around their frame loops,
// written ONCE: the group total an analysis block leaves (group_total, chain_sums_epilogue), the carry prologue that turns those totals into every
// chain's phase on entry to a synthesis block (carry_prologue), and the end-of-chain settle of the chains' overlaps for the kernels that keep their
// overlap-add accumulator in registers, one wavefront per chain (settle_overlap; k_synthesize_v2 / _v3).  The results are specified bit for bit
// (DESIGN.md 4.8): every family adds and folds in the order written here.
//
// A block is a GROUP of NCH consecutive chains of one channel.  Each chain has a stage of ( last bin + 1 ) doubles in its idle transform buffer; where
// that is differs per family, so the functions take `stage_at( w, bin )`: the LDS address of bin `bin` of the stage of chain `w` of the block.
//
// One copy is left beside its kernel: k_synthesize_v3 keeps carry_prologue's statements as its own text (the dft 1024 synthesis compiled with more scratch
// and ran 1.5-2 % slower through the call; pv_kernels_v3.h says so where the text stands).  A change to carry_prologue is repeated there.
// Not here (a later step): ChainOverlap (pv_kernels_eo.h; eo / team) -- its publish rule (two wavefronts per chain) and its indexing differ -- and the
// in-loop half of the v2 / v3 protocol (the peek at the tail word, the head prefetch under the last transform, the publish at frame i_pub).
#pragma once
#include "pv_kernels_fast.h"

namespace flanhip {

// Before a chain publishes its head's tag from inside the frame loop (k_synthesize_v2 / _v3): every store this wavefront has issued has retired.
// FLANHIP_PUBLISH_DRAIN=0 is the A/B partner (round 5's form: the compiler's counted wait for the next row as the only proof)
#ifndef FLANHIP_PUBLISH_DRAIN
#define FLANHIP_PUBLISH_DRAIN 1
#endif
__device__ __forceinline__ void publish_drain()
	{
	if constexpr( FLANHIP_PUBLISH_DRAIN != 0 ) asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
	else asm volatile( "" ::: "memory" );
	}

// 8-byte loads / stores that other XCDs' wavefronts see inside a launch (agent scope: the L2s of two XCDs are not coherent for ordinary accesses)
__device__ __forceinline__ void st_agent( cf * p, cf v )
	{
	unsigned long long bits; __builtin_memcpy( &bits, &v, 8 );
	__hip_atomic_store( reinterpret_cast<unsigned long long*>( p ), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
	}
__device__ __forceinline__ cf ld_agent( const cf * p )
	{
	const unsigned long long bits = __hip_atomic_load( reinterpret_cast<const unsigned long long*>( p ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
	cf v; __builtin_memcpy( &v, &bits, 8 );
	return v;
	}

// =================================================================================================================
// Analysis: the chains' staged sums, added and folded in chain order, are the group's total.  With one total per group the synthesis kernel can work
// out its own carries (a few dozen additions per bin) and the scan kernel between the two is not launched at all.
// LASTBIN: C (or N2) -- a row has LASTBIN + 1 bins; NT threads per block; NCH chains per block.  The barrier in front is the one the stages wait behind.
// =================================================================================================================
template<int LASTBIN, int NT, int NCH, class StageAt>
__device__ __forceinline__ void group_total( const AnalyzeParams & p, int channel, int groups, int group, StageAt stage_at )
	{
	__syncthreads();
	const int live = min( NCH, p.chains_per_channel - group * NCH );            // chains of this block that walked a chain of the channel
	double * gdst = p.group_sums + ( int64_t( channel ) * groups + group ) * ( LASTBIN + 1 );
	for( int bin = int( threadIdx.x ); bin <= LASTBIN; bin += NT )
		{
		double run = 0.0;
		for( int w = 0; w < live; ++w )
			{
			const double v = run + *stage_at( w, bin );
			run = ( __builtin_fabs( v ) < FLANHIP_FOLD_FAST_LIMIT ) ? fold_phase_fast( v ) : fold_phase_any( v );
			}
		gdst[bin] = run;
		}
	}

// One wavefront per chain, a lane owning the bin pairs ( k, C - k ), k = lane + 64 q, q < H, and lane 0 bin C/2 (k_analyze_v2 / _v3): the chain's sums,
// folded like phase_vocoder.cpp:59, go to the workspace (what k_phase_sums2 would compute) and -- staged in this wavefront's now idle transform
// buffer, `stage` = stage_at( own wavefront, 0 ) -- into the group's total; the NaN / Inf words of the launch ride along.
template<int C, int H, int NT, int WAVES, class StageAt>
__device__ __forceinline__ void chain_sums_epilogue( const AnalyzeParams & p, const double ( &sumk )[H], const double ( &summ )[H], double sumx, unsigned mmax,
                                                     bool active, int64_t chain, int lane, int channel, int groups, int group, double * stage, StageAt stage_at )
	{
	bool bad = mmax >= 0x7f800000u;
	auto fold = [&]( double sq ) -> double
		{
		bad |= !( __builtin_fabs( sq ) <= 1.7976931348623157e308 );              // a NaN / Inf frequency poisons its sum
		return ( __builtin_fabs( sq ) < FLANHIP_FOLD_FAST_LIMIT ) ? fold_phase_fast( sq ) : fold_phase_any( sq );
		};
	if( active )
		{
		double * dst = p.sums + chain * ( C + 1 );
		#pragma unroll
		for( int q = 0; q < H; ++q )
			{
			const double a = fold( sumk[q] ), b = fold( summ[q] );
			dst[lane + 64 * q] = a;             stage[lane + 64 * q] = a;
			dst[C - lane - 64 * q] = b;         stage[C - lane - 64 * q] = b;
			}
		const double vx = fold( sumx );
		if( lane == 0 ) { dst[C / 2] = vx; stage[C / 2] = vx; }
		}
	const bool any_bad = __any( bad );
	if( p.nan_out && lane == 0 && active )
		{
		// no clearing pass: the flag word is "set" when it equals this launch's epoch (written beside it by chain 0)
		if( chain == 0 ) { p.nan_out[2] = p.nan_epoch; p.nan_out[4] = p.nan_epoch; }   // [4]: the sums of this epoch are in the workspace
		if( any_bad ) p.nan_out[0] = p.nan_epoch;
		}
	if( p.group_sums ) group_total<C, NT, WAVES>( p, channel, groups, group, stage_at );
	}

// =================================================================================================================
// Synthesis with p.group_sums set: no scan over the chains ran.  `carry` still holds the chains' own sums, group_carry the running phase on entry to
// every group (a scan over the producer's group totals: 1 / NCH of the elements).  The running phase on entry to a chain = that, then the chains of
// its group before it, added and folded in order (phase_vocoder.cpp:57-59 modulo pi2: the prefix k_phase_scan2 forms, associated group-wise).
// One thread per bin, its NB bins side by side (independent dependency chains), along the chains of this group, leaving every chain's carries in that
// chain's stage.  Every load goes out ahead of the dependent additions: one memory round trip; `between()` runs once the chain sums and group_carry
// are requested and before anything waits for them (k_synthesize_v2: the request of the first MF row, which travels while the carries are
// worked out).  Ends behind a block barrier (which serves the tables of the kernel's prologue too): each family then reads its own stage back.
// BATCH: group totals in flight per bin in the arm without group_carry.
// =================================================================================================================
template<int LASTBIN, int NT, int NCH, int BATCH, class StageAt, class Between>
__device__ __forceinline__ void carry_prologue( const SynthParams & p, int channel, int groups, int group, StageAt stage_at, Between between )
	{
	const int tid = int( threadIdx.x );
	// x + y folded like phase_vocoder.cpp:59: the branch-free fold of the frame loop (pv_math.h) wherever it is exact, i.e. always but
	// for sums beyond 3e9 rad or NaN, which take the general routine
	auto fold = []( double r )
		{
		return ( __builtin_fabs( r ) < FLANHIP_FOLD_FAST_LIMIT ) ? fold_phase_loop( r ) : fold_phase_any( r );
		};
	const double * gs = ( p.group_carry ? p.group_carry : p.group_sums ) + int64_t( channel ) * groups * ( LASTBIN + 1 );
	const double * sums0 = p.carry + ( int64_t( channel ) * p.chains_per_channel + int64_t( group ) * NCH ) * ( LASTBIN + 1 );   // the first chain of this group
	const int live = min( NCH, p.chains_per_channel - group * NCH );
	constexpr int NB = ( LASTBIN + NT ) / NT;                                   // bins per thread (the last one only for thread 0)
	int bins_of[NB]; bool has[NB]; double run[NB];
	#pragma unroll
	for( int b = 0; b < NB; ++b ) { bins_of[b] = tid + NT * b; has[b] = bins_of[b] <= LASTBIN; if( !has[b] ) bins_of[b] = LASTBIN; run[b] = 0.0; }
	double vc[NB][NCH];                                                         // the chains of this group: requested first, used last
	#pragma unroll
	for( int b = 0; b < NB; ++b )
		{
		#pragma unroll
		for( int w = 0; w < NCH; ++w ) vc[b][w] = ( w < live ) ? sums0[int64_t( w ) * ( LASTBIN + 1 ) + bins_of[b]] : 0.0;
		}
	if( p.group_carry )
		{
		#pragma unroll
		for( int b = 0; b < NB; ++b ) run[b] = gs[int64_t( group ) * ( LASTBIN + 1 ) + bins_of[b]];   // the running phase on entry to this group (k_phase_scan2<SEG, true>)
		}
	between();
	if( !p.group_carry )
		{
		// few groups per channel (the host's choice): no scan over the group totals was launched -- this group adds up the totals of the groups
		// before it itself, BATCH loads per bin in flight (group g reads g totals: O(groups^2) bytes in all, cheaper than a kernel up to ~40 groups)
		for( int g0 = 0; g0 < group; g0 += BATCH )
			{
			double v[NB][BATCH];
			#pragma unroll
			for( int b = 0; b < NB; ++b )
				{
				#pragma unroll
				for( int u = 0; u < BATCH; ++u ) v[b][u] = ( g0 + u < group ) ? gs[int64_t( g0 + u ) * ( LASTBIN + 1 ) + bins_of[b]] : 0.0;
				}
			#pragma unroll
			for( int u = 0; u < BATCH; ++u )
				{
				#pragma unroll
				for( int b = 0; b < NB; ++b ) run[b] = fold( run[b] + v[b][u] );      // + 0.0 past the end: fold( x ) of a folded x is x
				}
			}
		}
	#pragma unroll
	for( int w = 0; w < NCH; ++w )
		{
		#pragma unroll
		for( int b = 0; b < NB; ++b )
			{
			if( has[b] ) *stage_at( w, bins_of[b] ) = run[b];                     // phase_buffer on entry to chain w of the group
			run[b] = fold( run[b] + vc[b][w] );
			}
		}
	if( tid == 0 && blockIdx.x == 0 )
		{
		if( p.nan_in && p.nan_flag && p.nan_in[0] == p.nan_in[2] && p.nan_in[2] != 0 ) atomicOr( p.nan_flag, 1 );
		if( p.expect_epoch && p.nan_in && p.nan_flag && p.nan_in[2] != p.expect_epoch ) atomicOr( p.nan_flag, 2 );   // the sums in this workspace are not the noted producer's
		if( p.skip_words ) const_cast<int*>( p.skip_words )[4] = 0;              // a handed-over pre-pass is good for one convert_to_audio (k_sums_and_groups has read the word: a launch ago)
		}
	__syncthreads();
	}

// =================================================================================================================
// Synthesis, p.fix_state set, the overlap-add accumulator in registers and one wavefront per chain (k_synthesize_v2 / _v3): the end of the chain.
// The overlaps of neighbouring chains are added by the chains themselves instead of by a launch of their own (k_ola_fixup: a launch and two round
// trips to memory behind every convert_to_audio).  The W - hop samples at a boundary get the LAST partial sums of the chain before it (in its `acc`
// when it ends) and the FIRST ones of the chain after it (in its `head` buffer since its first frames).  One word per boundary, tagged with the
// launch's epoch, written by atomic exchange; whoever finds the other side's tag there adds the two halves, so no wavefront ever waits for another
// and the order in which blocks are scheduled cannot matter.  The head's owner publishes INSIDE its frame loop, as soon as the loop's own counted
// wait has proven the head's stores acknowledged (memory operations retire in order); the tail's owner reads the word one frame before its last (the
// answer arrives under that frame's row wait), requests the head under its LAST transform (`hx`, `have_head`) and adds it to its accumulator as it
// leaves: no exchange, no round trip at the end of the launch.  That much stays in the kernels' frame loops; what follows the loop is here.  The
// halves cross XCDs inside a launch: written and read at agent scope (st_agent / ld_agent).  One addition per sample, tail + head, as k_ola_fixup
// does it: the same bits.
// acc[q] / hx[q] <-> samples pos + 128 q + 2 lane (+1); old_h: lane 0's, what the head word held before this chain's tag (if `published`).
// =================================================================================================================
template<int E>
__device__ __forceinline__ void settle_overlap( const SynthParams & p, const cf ( &acc )[E], cf ( &hx )[E], bool have_head, bool published, int old_h,
                                                bool has_head, bool has_tail, int64_t chain, int64_t chain_start, int64_t pos, int lane, cf * out2 )
	{
	const int tag_tail = p.fix_tag | 1, tag_head = p.fix_tag | 2;
	const int nsteps = p.head_len / 128;                                        // steps of 128 samples a boundary holds (W - hop, a multiple of 128 here)
	int * const word_h = p.fix_state + chain, * const word_t = p.fix_state + ( chain + 1 );
	const cf * const head_next = reinterpret_cast<const cf*>( p.head + ( chain + 1 ) * p.head_len ) + lane;
	if( has_head && !published )
		{
		// a chain too short to have published from its loop: now, behind a drained queue
		asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
		if( lane == 0 ) old_h = __hip_atomic_exchange( word_h, tag_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
		}
	if( has_tail )
		{
		// this chain's tail meets the next chain's head
		cf * tail_next = reinterpret_cast<cf*>( p.tail + ( chain + 1 ) * p.head_len ) + lane;
		bool add = have_head;
		if( !add )
			{
			// the neighbour had not published a frame ago (a launch of several rounds, a chain of one frame): leave the tail where it will
			// find it, BEHIND a drained queue, and say so; if its tag has appeared meanwhile the addition is ours after all
			#pragma unroll
			for( int q = 0; q < E; ++q ) if( q < nsteps ) st_agent( tail_next + 64 * q, acc[q] );
			asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
			int old = 0;
			if( lane == 0 ) old = __hip_atomic_exchange( word_t, tag_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
			add = __builtin_amdgcn_readfirstlane( old ) == tag_head;
			if( add )
				{
				#pragma unroll
				for( int q = 0; q < E; ++q ) hx[q] = ( q < nsteps ) ? ld_agent( head_next + 64 * q ) : mk( 0.0f, 0.0f );
				}
			}
		if( add )
			{
			#pragma unroll
			for( int q = 0; q < E; ++q )
				{
				const int64_t a = pos + 128 * q + 2 * lane;
				if( q < nsteps && a >= 0 && a < p.out_len ) out2[a >> 1] = mk( acc[q].x + hx[q].x, acc[q].y + hx[q].y );
				}
			}
		}
	if( has_head && __builtin_amdgcn_readfirstlane( old_h ) == tag_tail )
		{
		// this chain's head meets the previous chain's tail, which was there when the head's tag went out
		const cf * tl = reinterpret_cast<const cf*>( p.tail + chain * p.head_len ) + lane;
		const cf * hd = reinterpret_cast<const cf*>( p.head + chain * p.head_len ) + lane;
		#pragma unroll 4
		for( int q = 0; q < nsteps; ++q )
			{
			const cf t = ld_agent( tl + 64 * q ), h = ld_agent( hd + 64 * q );
			const int64_t a = chain_start + 128 * q + 2 * lane;
			if( a >= 0 && a < p.out_len ) out2[a >> 1] = mk( t.x + h.x, t.y + h.y );
			}
		}
	}

} // namespace flanhip
