// spectrum.hip -- Audio::synthesize_spectrum (Audio/AudioSynthesis.cpp:151-268): one period of N = 2^p frames made by ONE inverse real FFT over a
// harmonic spectrum with random phases, then read by the resampler loop of Wavetable::synthesize (wavetable.hip).  DESIGN.md section 4.24.
//   k_spec_fill / k_spec_fill_t   the usual pre-merge of a real inverse: bins k and C - k ( C = N/2 ) of X = r ( cos theta, sin theta ) give the points
//                   k and C - k of the C complex points Z whose complex inverse yields ( table[2n], table[2n+1] ).  They are stored CONJUGATED, so that
//                   the passes below are forward transforms of fft_device.h, and (the _t form) transposed for the two-pass split
//   k_spec_rows     transforms of contiguous length C2 <= 4096, one workgroup in LDS each.  C <= 4096: the one transform, written to the table.
//                   Above: C = C1 C2, row k1 holds Z[k1 + C1 k2]; the row's transform over k2 leaves A[k1][m2], which is multiplied by
//                   exp( +2 pi i k1 m2 / C ) on the way out ( k1 m2 < C: the exact dyadic argument needs no reduction )
//   k_spec_cols     C2 transforms of length C1 <= 512 over k1, a tile of 16 adjacent columns m2 per workgroup (every row of the tile one 128-byte
//                   segment), one wavefront per column and four columns per wavefront.  Output m1 C2 + m2 is the table's pair ( 2n, 2n + 1 ) in
//                   natural order.  (The last pass of a Cooley-Tukey split yields the most significant output digit, so it is the column pass that
//                   ends in natural order, and the row pass runs first over the transposed points.)
// Skipped bins ( harmonic == 0 ), which the reference leaves as whatever fftwf_alloc_complex returned, are ZERO here: the caller's mag holds 0 there.
// Every sum runs in a fixed order and nothing is atomic, so two runs agree bit for bit.
#include "flanhip_internal.h"
#include "fft_device.h"

#include <random>

namespace flanhip {

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_MIN_POWER = 6, SP_MAX_POWER = 22;
constexpr int SP_ROW_LOG2 = 12;                // the longest transform of one workgroup: 4096 complex points
constexpr int SP_TILE = 16;                    // columns per workgroup of the column pass, and the edge of the fill's transposing tile
constexpr float SP_RATE = 48000.0f;            // the table's sample rate (Audio::create_empty_with_frames' default)

struct SpSplit { int l1, l2; };                // C = 2^l1 2^l2; l1 == 0: one workgroup
SpSplit sp_split( int p )
	{
	const int lc = p - 1;
	if( lc <= SP_ROW_LOG2 ) return SpSplit{ 0, lc };
	const int l1 = std::max( 4, lc - SP_ROW_LOG2 );
	return SpSplit{ l1, lc - l1 };
	}

int sp_table_check( const void * mag, const void * theta, int32_t p, const void * table )
	{
	FLANHIP_REQUIRE( p >= SP_MIN_POWER && p <= SP_MAX_POWER, FLANHIP_ERR_UNSUPPORTED, "spectrum_size_power must lie in 6 ... 22" );
	FLANHIP_REQUIRE( mag && theta && table, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	return FLANHIP_OK;
	}

// The conjugates of Z[k] and Z[C - k], 0 <= k <= C/2.  E = X_k + conj( X_m ), D = X_k - conj( X_m ), O = D exp( +2 pi i k / N ), Z[k] = E + i O,
// Z[m] = conj( E ) + i conj( O ).  c2r ignores the imaginary parts of bins 0 and C.
__device__ __forceinline__ void sp_pair( const float * __restrict__ mag, const float * __restrict__ theta, int k, int C, cf * zk, cf * zm )
	{
	const int m = C - k;
	double sk, ck, sm, cm, sw, cw;
	sincos( double( theta[k] ), &sk, &ck );
	sincos( double( theta[m] ), &sm, &cm );
	sincospi( double( k ) / double( C ), &sw, &cw );                             // 2 k / N, exact
	const float rk = mag[k], rm = mag[m];
	cf xk = mk( rk * float( ck ), rk * float( sk ) ), xm = mk( rm * float( cm ), rm * float( sm ) );
	if( k == 0 ) { xk.y = 0.0f; xm.y = 0.0f; }
	const float ax = xk.x + xm.x, ay = xk.y - xm.y;
	const float dx = xk.x - xm.x, dy = xk.y + xm.y;
	const float cc = float( cw ), ss = float( sw );
	const float bx = __builtin_fmaf( cc, dx, -( ss * dy ) ), by = __builtin_fmaf( cc, dy, ss * dx );
	*zk = mk( ax - by, -( ay + bx ) );
	*zm = mk( ax + by, ay - bx );
	}

// C <= 4096: natural order.  grid: ( C/2 + 1 ) threads
__global__ __launch_bounds__( SP_THREADS ) void k_spec_fill( const float * __restrict__ mag, const float * __restrict__ theta, int C, cf * __restrict__ Z )
	{
	const int k = int( blockIdx.x ) * SP_THREADS + int( threadIdx.x );
	if( k > C / 2 ) return;
	cf zk, zm;
	sp_pair( mag, theta, k, C, &zk, &zm );
	Z[k] = zk;
	if( k != 0 && k != C - k ) Z[C - k] = zm;
	}

// C = C1 C2: point k = k1 + C1 k2 goes to k1 C2 + k2.  grid: ( C1 / 16 ) x ( C2 / 32 ) tiles of 16 k1 x 16 k2 with k2 < C2 / 2, which hold every
// pair once but k = C/2 ( k1 = 0, k2 = C2 / 2 ), its own partner: thread 0 of tile 0 adds it.  A tile is read along k1 (64-byte runs of mag and
// theta) and written along k2 (128-byte runs); the partners C - k = ( C1 - k1 ) + C1 ( C2 - 1 - k2 ), or C1 ( C2 - k2 ) in row 0, run backwards
__global__ __launch_bounds__( SP_THREADS ) void k_spec_fill_t( const float * __restrict__ mag, const float * __restrict__ theta, int l1, int l2,
	cf * __restrict__ Z )
	{
	__shared__ cf s_k[SP_TILE][SP_TILE + 1], s_m[SP_TILE][SP_TILE + 1];
	const int C1 = 1 << l1, C2 = 1 << l2, C = C1 * C2;
	const int tiles1 = C1 / SP_TILE;
	const int a = ( int( blockIdx.x ) % tiles1 ) * SP_TILE, b = ( int( blockIdx.x ) / tiles1 ) * SP_TILE;
	const int lo = int( threadIdx.x ) & ( SP_TILE - 1 ), hi = int( threadIdx.x ) >> 4;
		{
		const int k = ( a + lo ) + C1 * ( b + hi );
		cf zk, zm;
		sp_pair( mag, theta, k, C, &zk, &zm );
		s_k[hi][lo] = zk; s_m[hi][lo] = zm;
		}
	__syncthreads();
	const int k1 = a + hi, k2 = b + lo;
	Z[int64_t( k1 ) * C2 + k2] = s_k[lo][hi];
	if( k1 != 0 ) Z[int64_t( C1 - k1 ) * C2 + ( C2 - 1 - k2 )] = s_m[lo][hi];
	else if( k2 != 0 ) Z[C2 - k2] = s_m[lo][hi];
	if( blockIdx.x == 0 && threadIdx.x == 0 )
		{
		cf zk, zm;
		sp_pair( mag, theta, C / 2, C, &zk, &zm );
		Z[C2 / 2] = zk;
		}
	}

// grid: rows.  Z: cf[rows][C2] (conjugated points).  TWO: the result, times the inter-pass twiddle and conjugated again, back in place; else the
// result to table as float2[C2].  Dynamic LDS: cf buf[padded_len( C2 )], tw[C2]
template<int LOG2C, bool TWO>
__global__ __launch_bounds__( SP_THREADS ) void k_spec_rows( cf * __restrict__ Z, int l1, cf * __restrict__ table )
	{
	constexpr int C2 = 1 << LOG2C;
	extern __shared__ __align__( 16 ) char s_raw[];
	cf * buf = reinterpret_cast<cf*>( s_raw );
	cf * tw = buf + padded_len( C2 );
	const int lane = threadIdx.x;
	const int k1 = blockIdx.x;
	cf * row = Z + int64_t( k1 ) * C2;
	for( int i = lane; i < C2; i += SP_THREADS )
		{
		double sn, cs;
		sincospi( 2.0 * double( i ) / double( C2 ), &sn, &cs );
		tw[i] = mk( float( cs ), float( -sn ) );
		buf[PAD( i )] = row[i];
		}
	__syncthreads();
	fft_forward<LOG2C, SP_THREADS>( buf, tw, lane );                             // (ends with a barrier)
	for( int t = lane; t < C2; t += SP_THREADS )
		{
		const cf F = buf[PAD( t )];                                                  // the inverse of the points is conj( F )
		if constexpr( TWO )
			{
			// conj( conj( F ) w ) = F conj( w ), w = exp( +2 pi i k1 t / C )
			double sn, cs;
			sincospi( 2.0 * double( k1 * t ) / double( int64_t( C2 ) << l1 ), &sn, &cs );
			const float c = float( cs ), s = float( sn );
			row[t] = mk( __builtin_fmaf( F.x, c, F.y * s ), __builtin_fmaf( F.y, c, -( F.x * s ) ) );
			}
		else table[t] = mk( F.x, -F.y );
		}
	}

// grid: C2 / 16 tiles.  Y: cf[C1][C2] (conjugated), table: float2[C1 C2].  Dynamic LDS: cf buf[16][padded_len( C1 )], tw[C1]
template<int LOG2C>
__global__ __launch_bounds__( SP_THREADS ) void k_spec_cols( const cf * __restrict__ Y, int l2, cf * __restrict__ table )
	{
	constexpr int C1 = 1 << LOG2C;
	constexpr int STRIDE = padded_len( C1 );
	extern __shared__ __align__( 16 ) char s_raw[];
	cf * buf = reinterpret_cast<cf*>( s_raw );
	cf * tw = buf + SP_TILE * STRIDE;
	const int lane = threadIdx.x;
	const int64_t C2 = int64_t( 1 ) << l2;
	const int64_t m2 = int64_t( blockIdx.x ) * SP_TILE;
	for( int i = lane; i < C1; i += SP_THREADS )
		{
		double sn, cs;
		sincospi( 2.0 * double( i ) / double( C1 ), &sn, &cs );
		tw[i] = mk( float( cs ), float( -sn ) );
		}
	for( int i = lane; i < SP_TILE * C1; i += SP_THREADS )
		{
		const int col = i & ( SP_TILE - 1 ), k1 = i >> 4;
		buf[col * STRIDE + PAD( k1 )] = Y[k1 * C2 + m2 + col];
		}
	__syncthreads();
	const int wave = lane >> 6;
	for( int col = wave; col < SP_TILE; col += SP_THREADS / 64 ) fft_forward<LOG2C, 64>( buf + col * STRIDE, tw, lane & 63 );
	__syncthreads();
	for( int i = lane; i < SP_TILE * C1; i += SP_THREADS )
		{
		const int col = i & ( SP_TILE - 1 ), m1 = i >> 4;
		const cf F = buf[col * STRIDE + PAD( m1 )];
		table[m1 * C2 + m2 + col] = mk( F.x, -F.y );
		}
	}

size_t sp_rows_lds( int l2 ) { return sizeof( cf ) * size_t( padded_len( 1 << l2 ) + ( 1 << l2 ) ); }
size_t sp_cols_lds( int l1 ) { return sizeof( cf ) * size_t( SP_TILE * padded_len( 1 << l1 ) + ( 1 << l1 ) ); }

int launch_sp_table( const float * d_mag, const float * d_theta, int32_t p, float * d_table, void * d_ws, hipStream_t s )
	{
	const SpSplit sp = sp_split( p );
	const int C = 1 << ( p - 1 );
	cf * Z = static_cast<cf*>( d_ws );
	cf * T = reinterpret_cast<cf*>( d_table );
	if( sp.l1 == 0 )
		{
		if( int rc = launch_kernel( "spectrum_table", k_spec_fill, ( C / 2 + 1 + SP_THREADS - 1 ) / SP_THREADS, SP_THREADS, 0, s, d_mag, d_theta, C, Z ) ) return rc;
		#define SP_CASE( L ) case L: return launch_kernel( "spectrum_table", k_spec_rows<L, false>, 1, SP_THREADS, sp_rows_lds( L ), s, Z, 0, T );
		switch( sp.l2 )
			{
			SP_CASE( 5 ) SP_CASE( 6 ) SP_CASE( 7 ) SP_CASE( 8 ) SP_CASE( 9 ) SP_CASE( 10 ) SP_CASE( 11 ) SP_CASE( 12 )
			}
		#undef SP_CASE
		}
	else
		{
		const int64_t C1 = int64_t( 1 ) << sp.l1, C2 = int64_t( 1 ) << sp.l2;
		if( int rc = launch_kernel( "spectrum_table", k_spec_fill_t, ( C1 / SP_TILE ) * ( C2 / 2 / SP_TILE ), SP_THREADS, 0, s, d_mag, d_theta, sp.l1, sp.l2, Z ) ) return rc;
		int rc = FLANHIP_ERR_UNSUPPORTED;
		#define SP_CASE( L ) case L: rc = launch_kernel( "spectrum_table", k_spec_rows<L, true>, C1, SP_THREADS, sp_rows_lds( L ), s, Z, sp.l1, T ); break;
		switch( sp.l2 )
			{
			SP_CASE( 9 ) SP_CASE( 10 ) SP_CASE( 11 ) SP_CASE( 12 )
			}
		#undef SP_CASE
		if( rc ) return rc;
		#define SP_CASE( L ) case L: return launch_kernel( "spectrum_table", k_spec_cols<L>, C2 / SP_TILE, SP_THREADS, sp_cols_lds( L ), s, (const cf*) Z, sp.l2, T );
		switch( sp.l1 )
			{
			SP_CASE( 4 ) SP_CASE( 5 ) SP_CASE( 6 ) SP_CASE( 7 ) SP_CASE( 8 ) SP_CASE( 9 )
			}
		#undef SP_CASE
		}
	set_error( "spectrum_table: no kernel for spectrum_size_power %d", int( p ) );
	return FLANHIP_ERR_UNSUPPORTED;
	}

float sp_fundamental( int32_t fundamental_power ) { return float( std::pow( 2.0, double( fundamental_power ) ) ); }      // :176

// the workspace of the whole call: the table, the set_volume words, then whichever of the two stages needs more
struct SpCallLayout { size_t table_off, volume_off, stage_off, total; };
SpCallLayout sp_call_layout( int32_t p, size_t table_ws, size_t synth_ws, size_t volume_ws )
	{
	SpCallLayout l;
	l.table_off = 0;
	l.volume_off = sizeof( float ) << p;
	l.stage_off = ( l.volume_off + volume_ws + 255 ) & ~size_t( 255 );
	l.total = l.stage_off + std::max( table_ws, synth_ws );
	return l;
	}

// the arguments of the whole call, refused with the message of the stage that refuses them, and its workspace
int sp_call_args( int32_t p, int32_t fp, int64_t ch, int64_t out_frames, int64_t g, const float * freq, int64_t freq_count, SpCallLayout * l )
	{
	FLANHIP_REQUIRE( p >= SP_MIN_POWER && p <= SP_MAX_POWER, FLANHIP_ERR_UNSUPPORTED, "spectrum_size_power must lie in 6 ... 22" );
	FLANHIP_REQUIRE( fp > 0 && fp <= p, FLANHIP_ERR_INVALID_ARG, "fundamental_power must lie in 1 ... spectrum_size_power" );     // :164-166
	const double rate_out = double( sp_fundamental( fp ) );
	const size_t synth_ws = flanhip_spectrum_synth_workspace_bytes( p, rate_out, ch, out_frames, g, freq, freq_count );
	if( !synth_ws )
		{
		FLANHIP_REQUIRE( ch > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
		const int64_t rc = flanhip_spectrum_synth_plan( out_frames, rate_out, g, freq, freq_count, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
			nullptr, nullptr, nullptr );
		if( rc < 0 ) return int( rc );
		FLANHIP_REQUIRE( false, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
		}
	const size_t volume_ws = flanhip_audio_set_volume_workspace_bytes( ch, out_frames );
	FLANHIP_REQUIRE( volume_ws, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	*l = sp_call_layout( p, flanhip_spectrum_table_workspace_bytes( p ), synth_ws, volume_ws );
	return FLANHIP_OK;
	}

// table, synthesis, set_volume( 1 ) (:265) on one stream, nothing leaving the device in between
int launch_sp_call( const float * d_mag, const float * d_theta, int32_t p, int32_t fp, int64_t ch, int64_t out_frames, int64_t g, const float * freq,
	int64_t freq_count, float * d_out, void * d_ws, const SpCallLayout & l, void * stream )
	{
	float * d_table = ws_at<float>( d_ws, l.table_off );
	if( int rc = flanhip_spectrum_table_dev( d_mag, d_theta, p, d_table, ws_at<char>( d_ws, l.stage_off ), stream ) ) return rc;
	if( int rc = flanhip_spectrum_synth_dev( d_table, p, double( sp_fundamental( fp ) ), ch, out_frames, g, freq, freq_count, d_out,
		ws_at<char>( d_ws, l.stage_off ), stream ) ) return rc;
	return flanhip_audio_set_volume_dev( d_out, ch, out_frames, SP_RATE, nullptr, 1.0f, d_out, ws_at<char>( d_ws, l.volume_off ), stream );
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int64_t flanhip_spectrum_bins( int32_t spectrum_size_power, int32_t fundamental_power, int32_t * harmonic, float * freq, int64_t capacity )
	{
	if( spectrum_size_power < 1 || spectrum_size_power > 30 || fundamental_power < 0 || fundamental_power > 30 ) return 0;
	const int64_t B = ( int64_t( 1 ) << ( spectrum_size_power - 1 ) ) + 1;
	const float fundamental = sp_fundamental( fundamental_power );
	const int64_t fill = std::min<int64_t>( std::max<int64_t>( capacity, 0 ), B );
	for( int64_t b = 0; b < fill; ++b )
		{
		const float freq_c = float( b ) * SP_RATE / float( B );                      // :186: by the number of bins, not the transform's size
		if( freq ) freq[b] = freq_c;
		if( harmonic ) harmonic[b] = int32_t( std::round( freq_c / fundamental ) );  // :201
		}
	return B;
	}

int32_t flanhip_spectrum_num_harmonics( int32_t fundamental_power )
	{
	if( fundamental_power < 0 || fundamental_power > 30 ) return 0;
	return int32_t( std::ceil( SP_RATE / sp_fundamental( fundamental_power ) ) + 1 );                           // :188
	}

int flanhip_spectrum_phases( uint32_t seed, const int32_t * harmonic, int64_t bins, float * theta )
	{
	FLANHIP_REQUIRE( harmonic && theta, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( bins >= 0, FLANHIP_ERR_INVALID_ARG, "negative size" );
	std::mt19937 rng( seed );
	const float pi2 = std::acos( -1.0f ) * 2.0f;
	for( int64_t b = 0; b < bins; ++b )
		theta[b] = harmonic[b] != 0 ? std::uniform_real_distribution<float>( 0.0f, pi2 )( rng ) : 0.0f;      // :212
	return FLANHIP_OK;
	}

int32_t flanhip_spectrum_jump( int64_t channel, int64_t num_channels, int32_t spectrum_size_power )
	{
	if( num_channels <= 0 || channel < 0 || channel >= num_channels || spectrum_size_power < 0 || spectrum_size_power > 30 ) return 0;
	const int32_t wavelength = int32_t( 1 ) << spectrum_size_power;
	return int32_t( ( float( channel ) / float( num_channels ) ) * float( wavelength ) );                       // :236
	}

size_t flanhip_spectrum_table_workspace_bytes( int32_t spectrum_size_power )
	{
	if( spectrum_size_power < SP_MIN_POWER || spectrum_size_power > SP_MAX_POWER ) return 0;
	return sizeof( cf ) << ( spectrum_size_power - 1 );
	}

int flanhip_spectrum_table_dev( const float * d_mag, const float * d_theta, int32_t spectrum_size_power, float * d_table, void * d_workspace, void * stream )
	{
	if( int rc = sp_table_check( d_mag, d_theta, spectrum_size_power, d_table ) ) return rc;
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	return launch_sp_table( d_mag, d_theta, spectrum_size_power, d_table, d_workspace, (hipStream_t) stream );
	}

int flanhip_spectrum_table( const float * mag, const float * theta, int32_t spectrum_size_power, float * table, volatile int * cancel )
	{
	if( int rc = sp_table_check( mag, theta, spectrum_size_power, table ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const size_t bins = ( size_t( 1 ) << ( spectrum_size_power - 1 ) ) + 1;
	const float * d_mag = nullptr; const float * d_theta = nullptr; float * d_table = nullptr; void * d_ws = nullptr;
	if( int rc = call.in( mag, sizeof( float ) * bins, &d_mag ) ) return rc;
	if( int rc = call.in( theta, sizeof( float ) * bins, &d_theta ) ) return rc;
	if( int rc = call.out( table, sizeof( float ) << spectrum_size_power, &d_table ) ) return rc;
	if( int rc = call.scratch( flanhip_spectrum_table_workspace_bytes( spectrum_size_power ), &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_sp_table( d_mag, d_theta, spectrum_size_power, d_table, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

size_t flanhip_audio_synthesize_spectrum_workspace_bytes( int32_t spectrum_size_power, int32_t fundamental_power, int64_t num_channels, int64_t out_frames,
	int64_t granularity_frames, const float * freq, int64_t freq_count )
	{
	SpCallLayout l;
	if( sp_call_args( spectrum_size_power, fundamental_power, num_channels, out_frames, granularity_frames, freq, freq_count, &l ) ) return 0;
	return l.total;
	}

int flanhip_audio_synthesize_spectrum_dev( const float * d_mag, const float * d_theta, int32_t spectrum_size_power, int32_t fundamental_power,
	int64_t num_channels, int64_t out_frames, int64_t granularity_frames, const float * freq, int64_t freq_count, float * d_out, void * d_workspace,
	void * stream )
	{
	SpCallLayout l;
	if( int rc = sp_call_args( spectrum_size_power, fundamental_power, num_channels, out_frames, granularity_frames, freq, freq_count, &l ) ) return rc;
	FLANHIP_REQUIRE( d_mag && d_theta && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	return launch_sp_call( d_mag, d_theta, spectrum_size_power, fundamental_power, num_channels, out_frames, granularity_frames, freq, freq_count, d_out,
		d_workspace, l, stream );
	}

int flanhip_audio_synthesize_spectrum( const float * mag, const float * theta, int32_t spectrum_size_power, int32_t fundamental_power, int64_t num_channels,
	int64_t out_frames, int64_t granularity_frames, const float * freq, int64_t freq_count, float * out, volatile int * cancel )
	{
	SpCallLayout l;
	if( int rc = sp_call_args( spectrum_size_power, fundamental_power, num_channels, out_frames, granularity_frames, freq, freq_count, &l ) ) return rc;
	FLANHIP_REQUIRE( mag && theta && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const size_t bins = ( size_t( 1 ) << ( spectrum_size_power - 1 ) ) + 1;
	const float * d_mag = nullptr; const float * d_theta = nullptr; float * d_out = nullptr; void * d_ws = nullptr;
	if( int rc = call.in( mag, sizeof( float ) * bins, &d_mag ) ) return rc;
	if( int rc = call.in( theta, sizeof( float ) * bins, &d_theta ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( num_channels ) * size_t( out_frames ), &d_out ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_sp_call( d_mag, d_theta, spectrum_size_power, fundamental_power, num_channels, out_frames, granularity_frames, freq, freq_count, d_out,
		d_ws, l, nullptr ) ) return rc;
	return call.finish();
	}

} // extern "C"
