! Level fluxes through the Fortran shell: specifyParameters(computeLevelFluxes = .true.) and reportResults(levelFluxUp =,
! levelFluxDown =) on a small cloud over a reflecting surface, irregular layers.  Prints, per level, the two fluxes of every column
! (tests/test_gpu_level_fluxes.py runs the same photons through the Python mirror), and what the shell answers when the level
! fluxes are asked for without having been computed, or into arrays of the wrong shape.
program levelFluxTest
  use ErrorMessages
  use RandomNumbers
  use scatteringPhaseFunctions
  use opticalProperties
  use monteCarloIllumination
  use monteCarloRadiativeTransfer
  implicit none
  integer, parameter :: nx = 4, ny = 2, nz = 6, nPhotons = 50000
  type(ErrorMessage)         :: status
  type(domain)               :: cloud
  type(integrator)           :: mc, twin
  type(randomNumberSequence) :: randoms
  type(photonStream)         :: photons
  type(phaseFunction)        :: hg
  type(phaseFunctionTable)   :: table
  real    :: ext(nx, ny, nz), ssa(nx, ny, nz), up(nx, ny, nz + 1), down(nx, ny, nz + 1), wrong(nx, ny, nz)
  real    :: fluxUp(nx, ny), fluxDown(nx, ny), up2(nx, ny, nz + 1), down2(nx, ny, nz + 1)
  integer :: idx(nx, ny, nz), i, j, k

  hg = new_PhaseFunction(0.85**(/ (i, i = 1, 64) /), status = status)
  table = new_PhaseFunctionTable((/ hg /), key = (/ 1. /), status = status)
  do k = 1, nz
    do j = 1, ny
      do i = 1, nx
        ext(i, j, k) = 0.0002
        if(k >= 3 .and. k <= 5) ext(i, j, k) = 0.004 * (1 + mod(i + j, 3))
      end do
    end do
  end do
  ssa = 0.95; idx = 1
  cloud = new_Domain((/ 0., 500., 1000., 1500., 2000. /), (/ 0., 500., 1000. /), (/ 0., 100., 250., 300., 500., 800., 1000. /), status)
  call addOpticalComponent(cloud, "cloud", ext, ssa, idx, table, status = status)
  mc = new_Integrator(cloud, status)
  if(stateIsFailure(status)) then
    print *, "new_Integrator failed"; stop 1
  end if
  call specifyParameters(mc, surfaceAlbedo = 0.3, minInverseTableSize = 10001, status = status)

  ! asked for before they are switched on
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  call finalize_PhotonStream(photons)
  call initializeState(status)
  call reportResults(mc, status = status, levelFluxUp = up)
  print '(a, l2, 1x, a)', "unavailable ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  call specifyParameters(mc, status = status, computeLevelFluxes = .true.)
  if(stateIsFailure(status)) then
    print *, "specifyParameters(computeLevelFluxes) failed"; stop 1
  end if
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransfer failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportResults(mc, status = status, levelFluxUp = wrong)
  print '(a, l2, 1x, a)', "wrongshape  ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportResults(mc, fluxUp = fluxUp, fluxDown = fluxDown, status = status, levelFluxUp = up, levelFluxDown = down)
  if(stateIsFailure(status)) then
    print *, "reportResults failed: ", trim(failureText()); stop 1
  end if
  do k = 1, nz + 1
    print '(a, i3, 8f10.6)', "levelup   ", k - 1, ((up(i, j, k), i = 1, nx), j = 1, ny)
    print '(a, i3, 8f10.6)', "leveldown ", k - 1, ((down(i, j, k), i = 1, nx), j = 1, ny)
  end do
  print '(a, 8f10.6)', "fluxup    ", ((fluxUp(i, j), i = 1, nx), j = 1, ny)
  print '(a, 8f10.6)', "fluxdown  ", ((fluxDown(i, j), i = 1, nx), j = 1, ny)
  ! a copy made with the feature on: it reports the original's results, and the same batch through it gives them again
  twin = copy_Integrator(mc)
  call initializeState(status)
  call reportResults(twin, status = status, levelFluxUp = up2, levelFluxDown = down2)
  print '(a, l2, 2es10.2)', "copied      ", stateIsFailure(status), maxval(abs(up2 - up)), maxval(abs(down2 - down))
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(twin, randoms, photons, status)
  call finalize_PhotonStream(photons)
  up2 = -1.; down2 = -1.
  call initializeState(status)
  call reportResults(twin, status = status, levelFluxUp = up2, levelFluxDown = down2)
  print '(a, l2, 2es10.2)', "copyrun     ", stateIsFailure(status), maxval(abs(up2 - up)), maxval(abs(down2 - down))
  call finalize_Integrator(twin)
  ! switched off again: the arrays are gone
  call specifyParameters(mc, status = status, computeLevelFluxes = .false.)
  call initializeState(status)
  call reportResults(mc, status = status, levelFluxDown = down)
  print '(a, l2)', "offagain    ", stateIsFailure(status)
  call finalize_Integrator(mc)
  print '(a)', "level flux test done"
contains
  ! the oldest message of the status object (the probes start from a fresh one)
  function failureText() result(text)
    character(len = 256) :: text
    call firstMessage(status)
    text = getCurrentMessage(status)
  end function failureText
end program levelFluxTest
